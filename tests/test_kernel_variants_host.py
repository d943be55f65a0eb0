"""No GPU: tests/kernel_variants.py is complete and its test ids exist.

* every __global__ kernel instantiation of the built library (the dvae::__device_stub__ symbols `nm -C` lists: one host stub
  per instantiation; only NAMES are read) matches exactly one row of VARIANTS, and every row matches an instantiation -- a
  kernel added to csrc/ without a row, or a row left behind by a removed kernel, fails here;
* every row names a GPU test or a reason, every numeric switch two tests (or the reason no call reaches it, guarded by a host
  test), OPEN_SWITCHES is empty, and pytest collects every id named;
* TRIP_CLASSES: the launch arithmetic, evaluated at the image count of each named test, gives the trip-count class the table
  claims for it, and every required class of every persistent kernel family has a test;
* PREDICATES: every row cites a source line that holds its term, its neighbour is its base with the one named argument changed,
  it names two different tests (or the reason no call negates the term), and every ==, !=, % or alignment comparison on the
  launcher-condition lines of the conv and linear files is the term of some row;
* tools/kernel_trace_names.py reduces a kernel trace to the same spelling of the names."""
import os
import re
import shutil
import subprocess
import sys
from collections import Counter

import pytest

import kernel_variants as KV
from disvae_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_trace_names as KT  # noqa: E402

_STUB = re.compile(r"__device_stub__(\w+(?:<[^(]*>)?)\(")


def stub_names(nm_output):
    """demangled `nm -C` text -> sorted kernel instantiations, e.g. 'k_fc32<32, false, 0>'."""
    out = set()
    for line in nm_output.splitlines():
        m = _STUB.search(line.replace("(anonymous namespace)::", ""))
        if m:
            out.add(m.group(1))
    return sorted(out)


@pytest.fixture(scope="module")
def instantiations():
    lib = os.path.abspath(_lib.LIB_PATH)
    if not os.path.exists(lib):
        pytest.fail("libdvae_hip.so is not built (python disentangling-vae_amd/build.py)")
    nm = shutil.which("nm") or shutil.which("llvm-nm", path="/opt/rocm/llvm/bin")
    assert nm, "no nm on this machine"
    names = stub_names(subprocess.run([nm, "-C", lib], capture_output=True, text=True, check=True).stdout)
    assert len(names) > 100, names
    return names


def test_stub_name_parser():
    text = ("0000000000233c50 T dvae::__device_stub__k_adam(dvae::AdamTable, float, float)\n"
            "0000000000219070 W void dvae::__device_stub__k_up_thin<1, true, unsigned char>(float const*, int)\n"
            "00000000002357c0 t dvae::(anonymous namespace)::__device_stub__k_iw_loglik(float const*, long)\n"
            "0000000000000000 T dvae_version\n")
    assert stub_names(text) == ["k_adam", "k_iw_loglik", "k_up_thin<1, true, unsigned char>"]


def test_every_kernel_instantiation_has_exactly_one_row(instantiations):
    rows = Counter(v.kernel for v in KV.VARIANTS)
    twice = sorted(k for k, n in rows.items() if n > 1)
    assert not twice, "rows listed twice: %s" % twice
    missing = [k for k in instantiations if k not in rows]
    assert not missing, "kernel instantiations of the built library without a row in tests/kernel_variants.py: %s" % missing
    stale = sorted(k for k in rows if k not in instantiations)
    assert not stale, "rows of tests/kernel_variants.py that match no kernel of the built library: %s" % stale


def test_every_row_names_a_test_or_a_reason_and_cites_its_launch_site():
    csrc = os.path.join(ROOT, "disentangling-vae_amd", "csrc")
    lines = {}
    for v in KV.VARIANTS:
        assert (v.test is None) != (v.reason is None), v.kernel
        assert v.entry and v.when, v.kernel
        f, _, ln = v.where.partition(":")
        if f not in lines:
            with open(os.path.join(csrc, f)) as fh:
                lines[f] = fh.read().split("\n")
        assert 0 < int(ln) <= len(lines[f]) and lines[f][int(ln) - 1].strip(), (v.kernel, v.where)
        assert v.kernel.split("<")[0] in "\n".join(lines[f]), (v.kernel, v.where)     # (the line itself may be a launch macro's use)
    def cited(where):
        f, _, ln = where.partition(":")
        if f not in lines:
            with open(os.path.join(csrc, f)) as fh:
                lines[f] = fh.read().split("\n")
        return 0 < int(ln) <= len(lines[f]) and bool(lines[f][int(ln) - 1].strip())
    for s in KV.SWITCHES:
        assert s.launcher and s.variable and s.threshold, s
        assert cited(s.where), s
        if s.reason is None:
            assert s.below_test and s.above_test and s.below and s.above, s
            assert s.below_test != s.above_test, s                  # one test id PER SIDE
        else:                                                       # out of reach of the C-ABI: the argument, no half-filled pair
            assert s.below is s.above is s.below_test is s.above_test is None, s
            assert len(s.reason) > 80 and "test_kernel_variants_host.py::" in s.reason, s      # ... and the host test that guards it
            guard = s.reason.split("test_kernel_variants_host.py::")[1].split()[0]
            assert callable(globals().get(guard)), guard
    assert len({(s.launcher, s.variable, s.where) for s in KV.SWITCHES}) == len(KV.SWITCHES), "a switch is listed twice"
    assert KV.OPEN_SWITCHES == [], ("a threshold newly found in a launcher goes into SWITCHES with a test on either side of it (or "
                                    "the reason no call can reach it), not into OPEN_SWITCHES: %s" % (KV.OPEN_SWITCHES,))


def test_the_workspace_keeps_the_split_contraction_clamps_out_of_reach():
    """pick_split and launch_linear_wgrad (linear.hip:616, 718) halve the number of contraction slices while they do not fit the
    workspace.  capi.hip hands them dvae_conv_wgrad_ws_floats() floats, more than any slice count their first loops can ask for
    (KV.PICK_SPLIT_WS_BOUND: the SWITCHES row gives the argument), so no test sits at that flip -- if the workspace ever shrinks
    below the bound, this fails instead of the clamp being reached untested.  (Needs the library, not a GPU.)"""
    assert KV.PICK_SPLIT_WS_BOUND == 2162688
    def slices(tiles):                                              # pick_split's first loop on a contraction long enough never to end it
        S = 1
        while S < 16 and tiles * S < 256:
            S *= 2
        return S
    # (the clamp runs only while S > 1; an output of `tiles` 64x64 tiles has at most 4096 tiles elements)
    worst = max(slices(t) * (4096 * t + 4096) for t in range(1, 256))
    assert slices(256) == 1 and worst < KV.PICK_SPLIT_WS_BOUND, worst
    assert _lib.lib().dvae_conv_wgrad_ws_floats() >= KV.PICK_SPLIT_WS_BOUND


def _trip_counts(fam, N):
    """the trip count of every workgroup of `fam` at N images, by its expressions."""
    cdiv = lambda a, b: max(0, -(-a // b))
    grid = eval(fam.grid, {"N": N, "cdiv": cdiv, "min": min})
    return grid, [eval(fam.trips, {"N": N, "b": b, "grid": grid, "cdiv": cdiv}) for b in range(grid)]


def _trip_class(fam, N):
    grid, trips = _trip_counts(fam, N)
    lo, hi = min(trips), max(trips)
    assert lo >= 1 and sum(trips) > 0, (fam.family, N, "an idle workgroup")
    return "u%d" % lo if lo == hi else ("m%d" % lo if hi == lo + 1 else "spread %d..%d" % (lo, hi))


def test_trip_class_table_claims_what_the_launch_arithmetic_gives():
    csrc = os.path.join(ROOT, "disentangling-vae_amd", "csrc")
    assert len(KV.TRIP_CLASSES) == 10
    for fam in KV.TRIP_CLASSES:
        f, _, ln = fam.where.partition(":")
        with open(os.path.join(csrc, f)) as fh:
            line = fh.read().split("\n")[int(ln) - 1]
        assert "grid" in line, (fam.family, fam.where, line)        # the line that sizes the grid
        have = {}
        for cls, N, test in fam.cases:
            assert N >= fam.n_from, (fam.family, test)
            assert test.split("[")[1].split("-")[0].rstrip("]") == str(N), (fam.family, test, N)     # the id runs that image count
            assert _trip_class(fam, N) == cls, (fam.family, test, N, cls, _trip_class(fam, N))
            have.setdefault(cls, test)
        tmin = int(_trip_class(fam, fam.n_from)[1:])
        for t in range(tmin, fam.depth + 2):                        # every uniform count up to one past the pipeline depth
            if t in fam.unreachable:
                assert all(_trip_class(fam, N) != "u%d" % t for N in range(fam.n_from, 4097)), (fam.family, t)
            else:
                assert "u%d" % t in have, "%s: no test at %d trips in every workgroup" % (fam.family, t)
        above = [int(c[1:]) for c in have if c[0] == "u" and int(c[1:]) > fam.depth]
        assert any(t % 2 for t in above) and any(t % 2 == 0 for t in above), "%s: an odd and an even uniform count above depth %d" % (fam.family, fam.depth)
        assert any(c[0] == "m" for c in have), "%s: no mixed launch" % fam.family
    # the expressions themselves, at launches worked out by hand from the kernels
    by = {f.family: f for f in KV.TRIP_CLASSES}
    assert _trip_counts(by["k_down_thin_ws"], 193)[1].count(4) == 8 and _trip_counts(by["k_down_thin_ws"], 193)[1].count(3) == 504
    assert _trip_counts(by["k_wgrad_thin_ws"], 193)[1].count(7) == 8
    g, tr = _trip_counts(by["k_up_thin fused"], 193)                 # image 192 = lane 0 of the unit map: workgroups 0, 8, .. 56
    assert g == 1536 and [b for b in range(g) if tr[b] == 2] == list(range(0, 64, 8))
    assert _trip_counts(by["k_up_thin_mm"], 171) == (512, [2] + [1] * 511)
    assert _trip_counts(by["k_wgrad32ws (HS 16)"], 129)[0] == 192 and _trip_counts(by["k_wgrad32ws (HS 16)"], 321)[0] == 256


def test_every_named_test_is_collected():
    ids = ({v.test for v in KV.VARIANTS if v.test} | {t for s in KV.SWITCHES for t in (s.below_test, s.above_test) if t}
           | {c[2] for f in KV.TRIP_CLASSES for c in f.cases}
           | {t for r in KV.PREDICATES for t in (r.base_test, r.test) if t})
    assert all(i.startswith("tests/test_gpu_") for i in ids)
    files = sorted({i.split("::")[0] for i in ids})
    r = subprocess.run([sys.executable, "-m", "pytest", "--collect-only", "-q", "-p", "no:cacheprovider"] + files, cwd=ROOT,
                       capture_output=True, text=True)
    collected = {line.strip() for line in r.stdout.splitlines() if "::" in line}
    assert collected, r.stdout[-2000:] + r.stderr[-2000:]
    missing = sorted(ids - collected)
    assert not missing, "test ids named in tests/kernel_variants.py that pytest does not collect: %s" % missing


def _csrc_lines(f, cache={}):
    if f not in cache:
        with open(os.path.join(ROOT, "disentangling-vae_amd", "csrc", f)) as fh:
            cache[f] = fh.read().split("\n")
    return cache[f]


def test_every_predicate_row_cites_its_term_and_pairs_a_base_with_one_changed_argument():
    assert len(KV.PREDICATES) > 100
    for r in KV.PREDICATES:
        f, _, ln = r.where.partition(":")
        lines = _csrc_lines(f)
        assert 0 < int(ln) <= len(lines) and r.term in lines[int(ln) - 1], (r.where, r.term)
        assert r.launcher and r.term, r
        if r.reason is not None:                                    # no C-ABI call negates the term: the argument, no half-filled pair
            assert r.base is r.neighbour is r.arg is r.kernel is r.base_test is r.test is None and len(r.reason) > 40, r
            continue
        assert r.entry and r.kernel and r.family, r
        keys = set(r.arg.split(","))
        assert set(r.base) == set(r.neighbour), r
        assert {k for k in r.base if r.base[k] != r.neighbour[k]} == keys, (r.where, r.term, "the neighbour differs from the base in", r.arg)
        assert r.base_test and r.test and r.base_test != r.test, (r.where, r.term)
        if r.family in KV._FAMILY_TEST:                             # the ids are the ids of the two argument sets
            fn, ident = KV._FAMILY_TEST[r.family]
            assert r.base_test.endswith("::%s[%s]" % (fn, ident(r.base))) and r.test.endswith("::%s[%s]" % (fn, ident(r.neighbour))), r
    assert len({(r.where, r.term, r.launcher) for r in KV.PREDICATES}) == len(KV.PREDICATES), "a term is listed twice"


_CMP = re.compile(r"[A-Za-z_][\w.]*(?:\s*%\s*\d+)?\s*(?:==|!=)\s*[A-Za-z_0-9][\w.:]*")
_MOD = re.compile(r"[A-Za-z_][\w.]*\s*%\s*\d+")
_ALIGN = re.compile(r"&\s*(?:15|7)\b|aligned16\([^()]*\)")


def predicate_terms(line):
    """the ==, !=, % and alignment comparisons of one source line (comments dropped), as the source spells them."""
    line = line.split("//")[0]
    out = _CMP.findall(line)
    rest = _CMP.sub(" ", line)
    return out + _MOD.findall(rest) + _ALIGN.findall(rest)


def test_predicate_term_scanner():
    assert predicate_terms("  if (!(a.Cb == 32 && a.Hs == a.Ws && (a.Hs == 8 || a.Hs == 16) && a.l != DVAE_NHWC)) return 1;  // x == y") == [
        "a.Cb == 32", "a.Hs == a.Ws", "a.Hs == 8", "a.Hs == 16", "a.l != DVAE_NHWC"]
    assert predicate_terms("if (off || Kc < 256 || Kc % 4 || (b && N % 4)) return false;") == ["Kc % 4", "N % 4"]
    assert predicate_terms("const int v = N % 4 == 0 && (((uintptr_t)c | (uintptr_t)b) & 15) == 0;") == ["N % 4 == 0", "& 15"]
    assert predicate_terms("if (tuned && ws != nullptr && aligned16(small, ws)) x;") == ["ws != nullptr", "aligned16(small, ws)"]


def test_every_comparison_of_a_launcher_condition_has_a_predicate_row():
    """A term added to one of the scanned launcher conditions (KV.PREDICATE_LINES) has no row, and fails here until it gets its
    base / neighbour pair; a condition that moves takes its rows' `where` along (the first test above holds them to the text)."""
    rows = {}
    for r in KV.PREDICATES:
        rows.setdefault(r.where, []).append(r.term)
    scanned = set()
    for f, lns in KV.PREDICATE_LINES:
        lines = _csrc_lines(f)
        for ln in lns:
            where = "%s:%d" % (f, ln)
            scanned.add(where)
            found = predicate_terms(lines[ln - 1])
            assert found, (where, "no comparison on this line: PREDICATE_LINES is stale")
            for t in found:
                assert any(t in term for term in rows.get(where, ())), "%s: `%s` has no row in KV.PREDICATES" % (where, t)
    assert not sorted(set(rows) - scanned), "rows on lines that PREDICATE_LINES does not scan"


TRACE_SAMPLE = '''"Kind","Agent_Id","Queue_Id","Kernel_Id","Kernel_Name","Correlation_Id","Start_Timestamp","End_Timestamp"
"KERNEL_DISPATCH",4,1,10,"void dvae::k_fc32<32, false, 0>(float const*, long, float const*, long, float*, long, int, int, int, float const*, int, float const*, int)",1,100,200
"KERNEL_DISPATCH",4,1,11,"dvae::k_adam(dvae::AdamTable, float, float, float, float, float, float, float, float) [clone .kd]",2,300,400
"KERNEL_DISPATCH",4,1,10,"void dvae::k_fc32<32, false, 0>(float const*, long, float const*, long, float*, long, int, int, int, float const*, int, float const*, int)",3,500,600
"KERNEL_DISPATCH",4,1,12,"void at::native::vectorized_elementwise_kernel<4, at::native::FillFunctor<float>, std::array<char*, 1ul> >(int, at::native::FillFunctor<float>, std::array<char*, 1ul>)",4,700,800
"KERNEL_DISPATCH",4,1,13,"dvae::(anonymous namespace)::k_recon_rows(float const*, void const*, int, int, int, int, long, int, float*, float*).kd",5,900,950
"KERNEL_DISPATCH",4,1,14,"void dvae::k_up_thin<1, true, unsigned char>(float const*, int)",6,960,990
'''


def test_trace_reduction_tool(tmp_path):
    p = tmp_path / "x_kernel_trace.csv"
    p.write_text(TRACE_SAMPLE)
    seen = KT.reduce_trace(str(p))
    assert dict(seen) == {"k_fc32<32, false, 0>": 2, "k_adam": 1, "k_recon_rows": 1, "k_up_thin<1, true, unsigned char>": 1}
    rows = {v.kernel for v in KV.VARIANTS}
    assert set(seen) <= rows                                      # the tool spells names as the table does
    assert any(k.startswith("at::native::") for k in KT.reduce_trace(str(p), everything=True))
    out = tmp_path / "out.txt"
    assert KT.main(["sample=" + str(p), "--out", str(out)]) == 0
    text = out.read_text().split("\n")
    assert text[0] == "# sample: 4 kernels, 5 launches" and text[1].split() == ["1", "k_adam"]
    # an unlabelled path that contains '=' is a path; a label ends at the FIRST '='
    d = tmp_path / "a=b"
    d.mkdir()
    q = d / "y=z_kernel_trace.csv"
    q.write_text(TRACE_SAMPLE)
    assert KT.split_label(str(q)) == (str(q), str(q))
    assert KT.split_label("run1=" + str(q)) == ("run1", str(q))
    assert KT.split_label("plain.csv") == ("plain.csv", "plain.csv")
    assert KT.main([str(q), "--out", str(out)]) == 0 and out.read_text().startswith("# %s: 4 kernels" % q)


def test_committed_trace_shows_every_kernel_the_table_gives_to_the_new_file():
    """profiles/kernel_variant_trace.txt = tools/kernel_trace_names.py on a kernel trace of tests/test_gpu_kernel_variants.py
    alone: every kernel whose row names a test of that file was launched in that run, and every name in the trace has a row."""
    with open(os.path.join(ROOT, "profiles", "kernel_variant_trace.txt")) as f:
        seen = {line.split(None, 1)[1].strip() for line in f if line.strip() and not line.startswith("#")}
    claimed = {v.kernel for v in KV.VARIANTS if v.test and v.test.startswith(KV.V)}
    assert len(claimed) > 80
    assert not sorted(claimed - seen), "rows that name a test of the file, but the kernel is not in its trace"
    assert not sorted(seen - {v.kernel for v in KV.VARIANTS}), "traced kernels without a row"


def test_latent_math_has_one_home():
    """csrc/latent_math.h is the one definition of log 2 pi and of the stratified-sampling weight: no per-file copy grows back."""
    csrc = os.path.join(ROOT, "disentangling-vae_amd", "csrc")
    text = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h"))}
    assert [f for f, t in text.items() if "1.83787" in t] == ["latent_math.h"]
    defs = [(f, m.group(1)) for f, t in text.items() for m in re.finditer(r"^[ \w]*\bfloat\s+(log_w_ij\w*)\s*\(", t, re.M)]
    assert defs == [("latent_math.h", "log_w_ij")], defs
