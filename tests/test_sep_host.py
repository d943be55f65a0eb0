"""CPU: the host side of the SEPIN / WSEPIN separability scores -- the eleventh library's C-ABI (include/dvae_sep_hip.h ==
disvae_amd/_seplib.py == the built libdvae_sep_hip.so), its row of build.py's SCORE_PLUGIN_TARGETS (TARGETS, PLUGIN_TARGETS and the
31 sources untouched), the rules its source obeys, the refusal of bad arguments before any launch, the workspace size,
evaluate.separability_scores_from_entropies on hand-made entropies, the argument errors of Evaluator.compute_separability_scores
(those of compute_elbo_decomposition, before any device work) -- and the cancellation property of the grid tables that keeps the
GPU test of the same tables (tests/test_gpu_sep.py) meaningful: in fp32 the leave-one-out sum formed by ADDING the other terms
stays inside the per-sample tolerance, the sum formed as T - t_i misses it by orders of magnitude.

Measured here (fp32 terms and sums in numpy, logsumexp in fp64, S = 64, multiples of 2e-6 |ref| + 2e-6):
    grid (8, 8, 4)        adding 0.087    subtracting 7.3e3
    grid (16, 16)         adding 0.074    subtracting 5.2e4
    grid (6, 5, 4, 3, 2)  adding 0.115    subtracting 4.4e3
"""
import ctypes
import importlib.util
import json
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import sep_ref as R
import disvae_amd
from disvae_amd import _cabi, _evallib, _lib, _seplib
from disvae_amd import evaluate as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dvae_sep_hip.h")
CSRC = os.path.join(ROOT, "disentangling-vae_amd", "csrc")
SOURCE = "latent_loo.hip"
DUMMY = 1 << 20                                                   # aligned non-NULL address, never dereferenced
#       z      mean   logvar N  D  S  ws     logq   H      stream
LOO = [DUMMY, DUMMY, DUMMY, 5, 3, 4, DUMMY, DUMMY, DUMMY, None]
#        eps    logvar rows   N  D  S  H_cond_d stream
COND = [DUMMY, DUMMY, DUMMY, 5, 3, 4, DUMMY, None]


def _build():
    spec = importlib.util.spec_from_file_location("dvae_build_sep", os.path.join(ROOT, "disentangling-vae_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _nm(path, *flags):
    nm = shutil.which("nm") or shutil.which("llvm-nm", path="/opt/rocm/llvm/bin")
    assert nm, "no nm on this machine"
    return subprocess.run([nm] + list(flags) + [path], capture_output=True, text=True, check=True).stdout


# ---- 1. the library -----------------------------------------------------------------------------------------------------------
def test_header_ctypes_table_and_exports_agree(monkeypatch):
    declared = sorted(set(re.findall(r"\b(dvae_sep_[a-zA-Z0-9_]+)\s*\(", _header())))
    assert declared == sorted(_seplib.SIGNATURES)
    assert declared == sorted(["dvae_sep_version", "dvae_sep_last_error", "dvae_sep_loo_logq_ws_floats", "dvae_sep_loo_logq",
                               "dvae_sep_cond_terms"])
    exported = sorted(set(re.findall(r" T (dvae_\w+)", _nm(os.path.abspath(_seplib.LIB_PATH), "-D", "--defined-only"))))
    assert exported == declared
    assert re.findall(r" U (dvae_\w+)", _nm(os.path.abspath(_seplib.LIB_PATH), "-D")) == []
    kinds = {ctypes.c_void_p: "p", ctypes.c_int: "i", ctypes.c_long: "l"}
    for name, params in re.findall(r"\b(dvae_sep_[a-zA-Z0-9_]+)\s*\(([^)]*)\)", _header()):
        got = []
        for prm in [x.strip() for x in params.split(",") if x.strip() != "void"]:
            got.append("p" if "*" in prm else ("l" if prm.startswith("long") else "i"))
        assert got == [kinds[t] for t in _seplib.SIGNATURES[name]], name
    macros = {k: int(v) for k, v in re.findall(r"#define (DVAE_SEP_\w+) (\d+)", _header())}
    mirrored = {"DVAE_SEP_VERSION": _seplib.VERSION, "DVAE_SEP_MAX_D": _seplib.MAX_D, "DVAE_SEP_TEMPLATE_D": _seplib.TEMPLATE_D,
                "DVAE_SEP_GROUP": _seplib.GROUP, "DVAE_SEP_CHUNK": _seplib.CHUNK, "DVAE_SEP_MAX_CHUNKS": _seplib.MAX_CHUNKS}
    assert macros == mirrored                                            # every macro of the header, none besides
    assert _seplib.MAX_D >= 32
    assert _seplib.lib().dvae_sep_version() == _seplib.VERSION == 1
    assert os.path.basename(_seplib.LIB_PATH) == "libdvae_sep_hip.so"
    binding = open(_seplib.__file__).read()
    assert 'Binding.for_library("sep", SIGNATURES, _RESTYPE' in binding and "LIB_PATH = _binding.path" in binding
    assert _seplib._binding.last_error == "dvae_sep_last_error" and _seplib._binding.signatures is _seplib.SIGNATURES
    monkeypatch.setenv("DVAE_SEP_HIP_LIB", "/elsewhere/lib.so")              # the override, read when a binding is made
    assert _cabi.Binding.for_library("sep", {}, {}, "").path == "/elsewhere/lib.so"
    assert "separability_scores_from_entropies" in disvae_amd.__all__
    assert disvae_amd.separability_scores_from_entropies is E.separability_scores_from_entropies
    assert 4 * 256 * _seplib.MAX_D <= 64 * 1024                            # k_loo_lse_wide's LDS at the largest D


def test_build_has_the_third_list_and_the_other_two_are_unchanged():
    build = _build()
    assert [tuple(row) for row in build.SCORE_PLUGIN_TARGETS] == [("sep", ["latent_loo"], "dvae_sep_hip.h")]
    assert [tuple(row) for row in build.PLUGIN_TARGETS] == [("mmd", ["mmd_pairs"], "dvae_mmd_hip.h")]
    assert [n for n, _s, _h in build.TARGETS] == ["", "eval", "score", "info", "irs", "unsup", "udr", "dci", "dip"]
    assert "latent_loo" not in build.ALL_SOURCES and len(build.ALL_SOURCES) == 31
    isa = open(os.path.join(ROOT, "tools", "isa_identity.py")).read()
    assert "latent_loo" not in isa
    assert build.SEP_SOURCES == ["latent_loo"] and os.path.exists(os.path.join(build.SRC, "latent_loo.hip"))
    assert os.path.basename(build.SEP_LIB) == "libdvae_sep_hip.so" and os.path.exists(build.SEP_LIB)
    assert os.path.dirname(os.path.abspath(build.SEP_LIB)) == os.path.join(ROOT, "disentangling-vae_amd", "lib")
    assert sorted(os.path.basename(h) for h in build.SEP_HEADERS if "include" in h.split(os.sep)) == ["dvae_hip.h", "dvae_sep_hip.h"]
    assert {os.path.basename(h) for h in build.SEP_HEADERS} - {"dvae_hip.h", "dvae_sep_hip.h"} == \
        {f for f in os.listdir(CSRC) if f.endswith(".h")}
    assert build._target(*build.SCORE_PLUGIN_TARGETS[0])[3] == os.path.join(build.OBJ, "flags_sep.txt")
    assert os.path.exists(os.path.join(build.OBJ, "flags_sep.txt"))          # build() stamped it
    text = open(os.path.join(ROOT, "disentangling-vae_amd", "build.py")).read()
    assert "for name, sources, header in TARGETS + PLUGIN_TARGETS:" in text
    assert "for name, sources, header in SCORE_PLUGIN_TARGETS:" in text
    assert len(re.findall(r"^\s+_build_row\(", text, re.M)) == 2 and len(re.findall(r"\b_build_target\(", text)) == 2   # one helper, two loops
    libs = [f for f in os.listdir(os.path.dirname(os.path.abspath(build.SEP_LIB))) if re.fullmatch(r"libdvae(_\w+)?_hip\.so", f)]
    assert len(libs) == 11, sorted(libs)
    src = open(os.path.join(CSRC, SOURCE)).read()
    assert sorted(re.findall(r'^#include "([^"]+)"', src, re.M)) == ["../../include/dvae_sep_hip.h", "common.h", "last_error.h"]


def test_source_obeys_the_rules_of_the_shared_plumbing():
    src = open(os.path.join(CSRC, SOURCE)).read()
    assert len(re.findall(r'^#include "last_error\.h"', src, re.M)) == 1
    assert not re.search(r"\bthread_local\b", src) and not re.search(r"^void set_error\(", src, re.M)
    for name in ("put_f64", "get_f64", "chunks_of", "lesser"):
        assert not re.search(r"^[ \w]*\b(?:void|double|int|T)\s+%s\s*\([^;{]*\)\s*\{" % name, src, re.M), name
    code = re.sub(r"//[^\n]*", "", src.split("#include", 1)[1])
    assert not re.search(r"atomic", code)                                   # no atomics of any kind
    assert "while" not in code and "hipLaunchCooperativeKernel" not in src  # no spinning, no cooperative launch
    assert not re.search(r"hipMalloc|hipFree|hipMemcpy|hipMemset|Synchronize", src)    # the entry points only enqueue
    assert not re.search(r"1\.837877|0\.9189385", src)                      # log 2 pi has its one home in latent_math.h
    # the numerical rule: a leave-one-out sum is prefix + suffix; nothing subtracts a term from a total
    assert re.search(r"v\[d\] = pre \+ suf\[d\];", code) and re.search(r"v\[u\]\[j\] = pre \+ suf\[j\];", code)
    assert not re.search(r"-\s*t\[", code)


def _put(good, i, v):
    return good[:i] + [v] + good[i + 1:]


def test_bad_arguments_are_refused_before_a_launch_with_the_librarys_own_text():
    h = _seplib.lib()
    assert h is _seplib.lib()                                             # loaded once
    bad = [("dvae_sep_loo_logq", _put(LOO, i, None)) for i in (0, 1, 2, 6, 7, 8)]
    bad += [("dvae_sep_cond_terms", _put(COND, i, None)) for i in (0, 1, 2, 6)]
    for name, good, (iN, iD, iS) in (("dvae_sep_loo_logq", LOO, (3, 4, 5)), ("dvae_sep_cond_terms", COND, (3, 4, 5))):
        bad += [(name, _put(good, iD, 0)), (name, _put(good, iD, -1)), (name, _put(good, iD, _seplib.MAX_D + 1))]
        bad += [(name, _put(good, iN, 0)), (name, _put(good, iN, -1)), (name, _put(good, iS, 0)), (name, _put(good, iS, -1))]
    for name, args in bad:
        with pytest.raises(_lib.DvaeHipError) as e:
            _seplib.call(name, *args)
        own = h.dvae_sep_last_error().decode()
        assert "invalid argument" in own and SOURCE in own, (name, args, own)
        assert str(e.value) == "%s failed (-1): %s" % (name, own)
    with pytest.raises(_lib.DvaeHipError, match=r"D >= 1 && D <= DVAE_SEP_MAX_D"):       # the range, in the library's own words
        _seplib.call("dvae_sep_loo_logq", *_put(LOO, 4, _seplib.MAX_D + 1))
    assert SOURCE not in _evallib.lib().dvae_eval_last_error().decode()    # every library keeps its own buffer


def test_call_loads_through_the_modules_lib(monkeypatch):
    class Boom(Exception):
        pass

    def boom():
        raise Boom("lib() of the module was asked")
    monkeypatch.setattr(_seplib, "lib", boom)
    with pytest.raises(Boom, match="was asked"):
        _seplib.call("dvae_sep_loo_logq", *LOO)


def test_workspace_size_is_zero_out_of_range_and_monotone():
    ws = _seplib.lib().dvae_sep_loo_logq_ws_floats
    for N, D, S in ((0, 10, 5), (5, 0, 5), (5, 10, 0), (-1, 10, 5), (5, -3, 5), (5, 10, -7), (5, _seplib.MAX_D + 1, 5)):
        assert ws(N, D, S) == 0
    L = _seplib.CHUNK
    sizes = [1, 2, 7, 255, 256, 257, 1000, L - 1, L, L + 1, 10000, 10240, 10241, 65536, 100000, 737280, 1 << 22]
    for D in (1, 2, 4, 5, 10, 16, 17, _seplib.MAX_D):
        for a in sizes:
            row = [ws(a, D, b) for b in sizes]
            col = [ws(b, D, a) for b in sizes]
            assert row == sorted(row) and col == sorted(col), (D, a)
            assert row[0] >= a * 3 * D + 2 * (D + 1)              # the record table and one (max, sum) pair per row at the least
    assert ws(737280, 10, 10000) * 4 < 1 << 30                    # the dSprites shape: under 1 GiB


# ---- 2. the scores from hand-made entropies ------------------------------------------------------------------------------------
def _assert_matches_restatement(got, H_z, H_z_d, H_loo, H_cond_d):
    want = R.scores(H_z, H_z_d, H_loo, H_cond_d)
    assert set(got) == set(want)
    for k, v in want.items():
        np.testing.assert_allclose(got[k], v, rtol=1e-12, atol=1e-12, err_msg=k)
        assert isinstance(got[k], float) or (isinstance(got[k], list) and all(isinstance(x, float) for x in got[k])), k
    json.dumps(got)


def test_scores_of_an_independent_code():
    H_z_d, H_cond_d = [1.5, 0.25, 2.0, -0.5], [0.5, 0.25, -1.0, -0.75]
    H_z = math.fsum(H_z_d)
    H_loo = [H_z - h for h in H_z_d]
    got = E.separability_scores_from_entropies(H_z, H_z_d, H_loo, H_cond_d)
    _assert_matches_restatement(got, H_z, H_z_d, H_loo, H_cond_d)
    assert max(abs(v) for v in got["redundancy"]) <= 1e-15 and abs(got["dtc"]) <= 1e-14 and abs(got["tc"]) <= 1e-15
    np.testing.assert_allclose(got["sepin"], got["informativeness"], rtol=0, atol=1e-14)
    np.testing.assert_allclose(got["informativeness"], [1.0, 0.0, 3.0, 0.25], rtol=0, atol=1e-15)
    np.testing.assert_allclose(got["rho"], [1 / 4.25, 0.0, 3 / 4.25, 0.25 / 4.25], rtol=1e-15)
    assert math.fsum(got["rho"]) == pytest.approx(1.0, abs=1e-15)
    assert got["wsepin"] == pytest.approx((1.0 + 9.0 + 0.0625) / 4.25, rel=1e-14)
    np.testing.assert_allclose(got["sepin_at_k"], [3.0, 2.0, 4.25 / 3, 4.25 / 4], rtol=1e-14)


def test_scores_of_one_dimension():
    got = E.separability_scores_from_entropies(1.25, [1.25], [0.0], [0.5])
    _assert_matches_restatement(got, 1.25, [1.25], [0.0], [0.5])
    assert got["sepin"] == [0.75] and got["informativeness"] == [0.75] and got["redundancy"] == [0.0]
    assert got["mi"] == 0.75 and got["mi_loo"] == [0.0] and got["rho"] == [1.0] and got["wsepin"] == 0.75
    assert got["sepin_at_k"] == [0.75] and got["dtc"] == 0.0 and got["tc"] == 0.0


def test_scores_identity_running_mean_and_weights():
    rng = np.random.RandomState(7)
    for D in (2, 3, 10, 33):
        H_z_d, H_loo, H_cond_d = rng.uniform(-2, 4, D), rng.uniform(-5, 20, D), rng.uniform(-4, 1, D)
        H_z = float(rng.uniform(-5, 20))
        got = E.separability_scores_from_entropies(H_z, H_z_d, H_loo, H_cond_d)
        _assert_matches_restatement(got, H_z, H_z_d, H_loo, H_cond_d)
        diff = np.array(got["informativeness"]) - np.array(got["redundancy"])
        np.testing.assert_allclose(got["sepin"], diff, rtol=0, atol=1e-13)              # sepin = informativeness - redundancy
        np.testing.assert_allclose(got["sepin"], H_z - H_loo - H_cond_d, rtol=0, atol=1e-13)
        ranked = sorted(got["sepin"], reverse=True)
        assert got["sepin_at_k"] == [math.fsum(ranked[:k]) / k for k in range(1, D + 1)]
        assert got["sepin_at_k"][0] == max(got["sepin"]) and got["sepin_at_k"][-1] == pytest.approx(np.mean(got["sepin"]), abs=1e-13)
        assert math.fsum(got["rho"]) == pytest.approx(1.0, abs=1e-14) and min(got["rho"]) >= 0.0
        assert [r == 0.0 for r in got["rho"]] == [v <= 0 for v in got["informativeness"]]
        assert got["wsepin"] == pytest.approx(float(np.dot(got["rho"], got["sepin"])), abs=1e-13)
    # nothing but rho is clamped: negative estimates stay negative
    got = E.separability_scores_from_entropies(1.0, [0.5, 0.5], [0.75, 0.5], [0.75, 0.25])
    assert got["informativeness"] == [-0.25, 0.25] and got["sepin"] == [-0.5, 0.25] and got["rho"] == [0.0, 1.0]
    assert got["wsepin"] == 0.25 and got["mi_loo"] == [0.5, -0.25]


def test_scores_without_any_informative_latent_are_zero_not_nan():
    got = E.separability_scores_from_entropies(1.0, [0.5, 0.25], [0.5, 0.75], [0.5, 1.0])       # informativeness 0 and -0.75
    assert got["rho"] == [0.0, 0.0] and got["wsepin"] == 0.0
    assert not any(math.isnan(v) for k in ("sepin", "rho", "sepin_at_k", "informativeness", "redundancy") for v in got[k])
    with pytest.raises(ValueError, match="one entropy per latent dimension"):
        E.separability_scores_from_entropies(1.0, [0.5, 0.25], [0.5], [0.5, 1.0])
    with pytest.raises(ValueError, match="one entropy per latent dimension"):
        E.separability_scores_from_entropies(1.0, [], [], [])


def test_scores_of_a_duplicated_latent_pair():
    """z_1 = z_0 among well-separated posteriors: the pair's joint entropy is the entropy of one of them plus its conditional
    entropy (the estimator takes the two as independent given x), so neither tells anything the other does not."""
    h0, c0, h2, c2 = 1.75, -3.5, 1.25, -3.0
    H_z_d, H_cond_d = [h0, h0, h2], [c0, c0, c2]
    H_z = h0 + c0 + h2                                            # H(z_0, z_1) = H(z_0) + H(z_1 | x)
    H_loo = [h0 + h2, h0 + h2, h0 + c0]
    got = E.separability_scores_from_entropies(H_z, H_z_d, H_loo, H_cond_d)
    _assert_matches_restatement(got, H_z, H_z_d, H_loo, H_cond_d)
    assert abs(got["sepin"][0]) <= 1e-14 and abs(got["sepin"][1]) <= 1e-14
    assert got["informativeness"][0] == h0 - c0 and got["sepin"][2] == pytest.approx(h2 - c2, abs=1e-14)
    assert got["redundancy"][0] == pytest.approx(h0 - c0, abs=1e-14)         # all it tells, the other tells too


# ---- 3. the cancellation property of the grid tables ---------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", R.GRIDS, ids=lambda s: "x".join(map(str, s)))
def test_adding_form_holds_the_tolerance_and_the_subtracting_form_misses_it(sizes):
    mean, logvar, rows, eps = R.grid_table(sizes, 64, seed=1)
    assert mean.shape == logvar.shape == (int(np.prod(sizes)), len(sizes)) and mean.dtype == logvar.dtype == np.float32
    assert len(set(rows.tolist())) == 64 and eps.shape == (64, len(sizes))
    assert -10.0 <= logvar.min() and logvar.max() <= -9.5
    np.testing.assert_allclose(mean, 3.0 * R.grid_digits(sizes), atol=0.05 * 6 * math.exp(-4.75))
    z = R.sample_z(mean, logvar, rows, eps)
    ref = R.loo_logq(z, mean, logvar)[:len(sizes)]
    assert np.isfinite(ref).all()
    adding = R.tolerance_multiple(R.fp32_loo_logq(z, mean, logvar, subtract=False), ref)
    subtracting = R.tolerance_multiple(R.fp32_loo_logq(z, mean, logvar, subtract=True), ref)
    print("grid %s: adding form %.3g x tolerance, subtracting form %.3g x tolerance" % (sizes, adding, subtracting))
    assert adding <= 1.0
    assert subtracting >= 100.0


def test_restatement_pieces():
    """np.delete-style sums against a literal loop, D = 1 (the empty sum), a sample without any finite density, and the product
    table: its aggregate posterior is the product of its marginals."""
    rng = np.random.RandomState(3)
    mean, logvar, z = rng.randn(6, 3), rng.uniform(-2, 0, (6, 3)), rng.randn(4, 3)
    got = R.loo_logq(z, mean, logvar)
    for i in range(4):
        keep = [[d for d in range(3) if d != i], [0, 1, 2]][i == 3]
        for s in range(4):
            dens = [sum(-0.5 * (R.LOG2PI + logvar[n, d]) - 0.5 * (z[s, d] - mean[n, d]) ** 2 * math.exp(-logvar[n, d]) for d in keep)
                    for n in range(6)]
            assert got[i, s] == pytest.approx(math.log(sum(math.exp(v) for v in dens)) - math.log(6), abs=1e-12)
    one = R.loo_logq(z[:, :1], mean[:, :1], logvar[:, :1])
    assert one.shape == (2, 4) and (one[0] == 0.0).all()
    np.testing.assert_allclose(one[1], R.marginal_logq(z[:, :1], mean[:, :1], logvar[:, :1])[0], rtol=1e-14)
    far = z.copy()
    far[2, 1] = 1e200
    with np.errstate(over="ignore"):
        inf = R.loo_logq(far, mean, logvar)
    assert not np.isnan(inf).any() and inf[0, 2] == inf[2, 2] == inf[3, 2] == -np.inf and np.isfinite(inf[1, 2])
    assert R.tolerance_multiple(inf, inf) == 0.0 and R.tolerance_multiple(np.where(np.isfinite(inf), inf, 0.0), inf) == np.inf
    mean, logvar, rows, eps = R.grid_table((4, 3, 2), 24, seed=2, product=True)
    ref = R.evaluation(R.sample_z(mean, logvar, rows, eps), eps, rows, mean, logvar)
    atol = R.derived_atol(ref)
    assert np.abs(ref["redundancy"]).max() <= atol and abs(ref["dtc"]) <= atol and abs(ref["tc"]) <= atol
    np.testing.assert_allclose(ref["sepin"], ref["informativeness"], rtol=0, atol=atol)
    # (z is rounded to fp32 at |z| up to 9 with sigma = 7e-3: the eps that z implies differs from the eps given by 1e-4 of itself)
    np.testing.assert_allclose(ref["informativeness"], np.log([4, 3, 2]), atol=1e-4)


# ---- 4. Evaluator: the errors of compute_elbo_decomposition, before any device work ----------------------------------------------
class _Model(torch.nn.Module):
    def __init__(self, dim=2):
        super().__init__()
        self.latent_dim, self.modes = dim, []

    def encoder(self, x):
        self.modes.append(self.training)
        return x[:, :1] + torch.zeros(1, self.latent_dim), torch.zeros(x.shape[0], self.latent_dim)


class _Loader:
    def __init__(self, rows, yields=None):
        self.dataset, self.rows = list(range(rows)), rows if yields is None else yields

    def __iter__(self):
        for lo in range(0, self.rows, 4):
            yield torch.arange(lo, min(lo + 4, self.rows), dtype=torch.float32).view(-1, 1), None


ERRORS = [
    (dict(n_samples=0), False),
    (dict(n_samples=7), False),
    (dict(n_samples=3, eps=torch.zeros(2, 2)), False),
    (dict(sample_idx=[0, 6]), False),
    (dict(n_samples=7, eps=torch.zeros(2, 2)), False),
    (dict(sample_idx=[0, 1, 2, 3, 4, 5, 0]), False),
]


@pytest.mark.parametrize("kw, encoded", ERRORS, ids=[str(i) for i in range(len(ERRORS))])
def test_evaluator_argument_errors_are_those_of_the_elbo_decomposition(monkeypatch, kw, encoded):
    def boom(*a, **k):
        raise AssertionError("device work before the refusal")
    monkeypatch.setattr(_seplib, "lib", boom)
    monkeypatch.setattr(_lib, "lib", boom)
    texts = []
    for method in ("compute_elbo_decomposition", "compute_separability_scores"):
        model = _Model().train()
        ev = E.Evaluator(model, None, is_progress_bar=False)
        with pytest.raises(ValueError) as e:
            getattr(ev, method)(_Loader(6), **kw)
        texts.append(str(e.value))
        assert model.training and bool(model.modes) == encoded
    assert texts[0] == texts[1] and texts[0]


def test_evaluator_refuses_a_short_loader_and_too_many_dimensions(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("device work before the refusal")
    monkeypatch.setattr(_seplib, "lib", boom)
    monkeypatch.setattr(_lib, "lib", boom)
    texts = []
    for method in ("compute_elbo_decomposition", "compute_separability_scores"):
        model = _Model().train()
        with pytest.raises(ValueError) as e:
            getattr(E.Evaluator(model, None, is_progress_bar=False), method)(_Loader(6, yields=5), n_samples=3)
        texts.append(str(e.value))
        assert model.training and model.modes == [False, False]           # encoded in eval mode, mode restored
    assert texts[0] == texts[1] == "the loader yielded 5 images, its data set has 6"
    model = _Model(_seplib.MAX_D + 1).train()
    with pytest.raises(ValueError) as e:
        E.Evaluator(model, None, is_progress_bar=False).compute_separability_scores(_Loader(6), n_samples=3)
    assert str(e.value) == "%d latent dimensions: the separability kernels take at most %d" % (_seplib.MAX_D + 1, _seplib.MAX_D)
    assert model.training and model.modes == []                           # before the encode pass


def test_call_writes_the_separability_scores_on_request(monkeypatch, tmp_path):
    seen = []
    model = _Model().train()
    ev = E.Evaluator(model, None, is_progress_bar=False, save_dir=str(tmp_path))
    result = {"sepin": [0.5, 0.25], "wsepin": 0.375, "n_samples": 11}
    monkeypatch.setattr(ev, "compute_separability_scores", lambda loader, **kw: seen.append((loader, kw, model.training)) or result)
    monkeypatch.setattr(ev, "compute_losses", lambda loader: {"loss": 1.5})
    loader = object()
    assert ev(loader) == (None, {"loss": 1.5}) and seen == [] and os.listdir(tmp_path) == ["test_losses.log"]
    assert ev(loader, is_losses=False, is_separability=True, n_samples_separability=11) == (None, None)
    assert seen == [(loader, dict(n_samples=11), False)] and model.training
    assert E.SEPARABILITY_SCORES_FILE == "separability_scores.log"
    assert json.load(open(tmp_path / "separability_scores.log")) == result
    ev(loader, is_losses=False, is_separability=True)
    assert seen[-1] == (loader, dict(n_samples=10000), False)
