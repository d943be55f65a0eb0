"""CPU: the host side of the unsupervised disentanglement ranking -- the seventh library's C-ABI (include/dvae_udr_hip.h ==
disvae_amd/_udrlib.py == the built libdvae_udr_hip.so), its row of build.py's TARGETS, the fp64 restatement
(tests/udr_ref.py) against scipy and sklearn where they exist, the pair and model scores on hand-made matrices, the host
combination of evaluate.py against the restatement, the precondition of the GPU tests' bounds, and the argument errors raised
before any library load.

The Lasso of the restatement against sklearn.linear_model.Lasso(alpha, tol=1e-12, max_iter=100000) on the standardised, masked
data: the worst coefficient difference over LASSO_CASES measured on the CPU is 6.4e-13 (sklearn stops on its duality gap, the
restatement on the largest coefficient change of a sweep); 100 x that is allowed, and never more
than 1e-8."""
import ctypes
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import udr_ref as R
import disvae_amd
from disvae_amd import _cabi, _lib, _udrlib, _unsuplib
from disvae_amd import evaluate as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dvae_udr_hip.h")
CSRC = os.path.join(ROOT, "disentangling-vae_amd", "csrc")
LASSO_WORST = 6.4e-13                                            # measured (module docstring)
LASSO_CASES = [(4096, 5, 4, 0.1, 0), (1000, 10, 10, 0.1, 1), (300, 3, 6, 0.02, 2), (2000, 8, 8, 0.3, 3)]   # (S, Dx, Dy, alpha, seed)


def _build():
    spec = importlib.util.spec_from_file_location("dvae_build_udr", os.path.join(ROOT, "disentangling-vae_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- 1. the library -----------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _nm(path, *flags):
    nm = shutil.which("nm") or shutil.which("llvm-nm", path="/opt/rocm/llvm/bin")
    assert nm, "no nm on this machine"
    return subprocess.run([nm] + list(flags) + [path], capture_output=True, text=True, check=True).stdout


def test_header_ctypes_table_and_exports_agree(monkeypatch):
    declared = sorted(set(re.findall(r"\b(dvae_udr_[a-zA-Z0-9_]+)\s*\(", _header())))
    assert declared == sorted(_udrlib.SIGNATURES) and len(declared) == 6
    assert declared == sorted(["dvae_udr_version", "dvae_udr_last_error", "dvae_udr_ranks_ws_floats", "dvae_udr_ranks",
                               "dvae_udr_kl_dims_ws_floats", "dvae_udr_kl_dims"])
    exported = sorted(set(re.findall(r" T (dvae_\w+)", _nm(os.path.abspath(_udrlib.LIB_PATH), "-D", "--defined-only"))))
    assert exported == declared
    kinds = {ctypes.c_void_p: "p", ctypes.c_int: "i", ctypes.c_long: "l"}
    for name, params in re.findall(r"\b(dvae_udr_[a-zA-Z0-9_]+)\s*\(([^)]*)\)", _header()):
        got = []
        for prm in [x.strip() for x in params.split(",") if x.strip() != "void"]:
            got.append("p" if "*" in prm else ("l" if prm.startswith("long") else "i"))
        assert got == [kinds[t] for t in _udrlib.SIGNATURES[name]], name
    macros = {k: int(v) for k, v in re.findall(r"#define (DVAE_UDR_\w+) (\d+)", _header())}
    mirrored = {"DVAE_UDR_VERSION": _udrlib.VERSION, "DVAE_UDR_MAX_D": _udrlib.MAX_D, "DVAE_UDR_MAX_ROWS": _udrlib.MAX_ROWS,
                "DVAE_UDR_SMALL_ROWS": _udrlib.SMALL_ROWS, "DVAE_UDR_CHUNK_ROWS": _udrlib.CHUNK_ROWS,
                "DVAE_UDR_MAX_CHUNKS": _udrlib.MAX_CHUNKS, "DVAE_UDR_KL_BLOCK_ROWS": _udrlib.KL_BLOCK_ROWS,
                "DVAE_UDR_KL_MAX_CHUNKS": _udrlib.KL_MAX_CHUNKS}
    assert macros == mirrored                                            # every macro of the header, none besides
    assert _udrlib.MAX_ROWS == 2 ** 23 and np.float32(2 ** 23 - 0.5) == 2 ** 23 - 0.5      # every half-integer rank is an fp32 number
    assert _udrlib.SMALL_ROWS * 16 + 6 * 1024 <= 64 * 1024             # two (key, row) buffers and the counters stay below 64 KB of LDS
    assert _udrlib.MAX_CHUNKS <= 256                                     # one chunk record per thread of the last launch
    assert _udrlib.lib().dvae_udr_version() == _udrlib.VERSION == 1
    assert os.path.basename(_udrlib.LIB_PATH) == "libdvae_udr_hip.so"
    binding = open(_udrlib.__file__).read()
    assert 'Binding.for_library("udr", SIGNATURES, _RESTYPE' in binding and "LIB_PATH = _binding.path" in binding
    assert _udrlib._binding.last_error == "dvae_udr_last_error" and _udrlib._binding.signatures is _udrlib.SIGNATURES
    monkeypatch.setenv("DVAE_UDR_HIP_LIB", "/elsewhere/lib.so")              # the override, read when a binding is made
    assert _cabi.Binding.for_library("udr", {}, {}, "").path == "/elsewhere/lib.so"
    assert "udr_from_tables" in disvae_amd.__all__ and disvae_amd.udr_from_tables is E.udr_from_tables


def test_udr_row_is_a_row_of_the_build_table():
    """what test_build_table_drives_the_exported_names_and_the_identity_tool demands of every row of TARGETS, of the udr row"""
    build = _build()
    rows = [row for row in build.TARGETS if row[0] == "udr"]
    assert [tuple(row) for row in rows] == [("udr", ["latent_ranks"], "dvae_udr_hip.h")]
    taken = {s for n, sources, _h in build.TARGETS if n != "udr" for s in sources}
    text = {f: open(os.path.join(CSRC, f)).read() for f in os.listdir(CSRC) if f.endswith((".hip", ".h"))}
    for name, sources, header in rows:
        prefix = name.upper() + "_"
        lib, srcs, headers = (getattr(build, prefix + suffix) for suffix in ("LIB", "SOURCES", "HEADERS"))
        assert srcs == sources and all(os.path.exists(os.path.join(build.SRC, s + ".hip")) for s in srcs)
        assert os.path.basename(lib) == "libdvae_%s_hip.so" % name
        assert os.path.dirname(os.path.abspath(lib)) == os.path.join(ROOT, "disentangling-vae_amd", "lib")
        assert header == "dvae_%s_hip.h" % name
        assert sorted(os.path.basename(h) for h in headers if "include" in h.split(os.sep)) == sorted({"dvae_hip.h", header})
        assert all(os.path.exists(h) for h in headers)
        csrc_headers = {os.path.basename(h) for h in headers} - {"dvae_hip.h", header}
        assert csrc_headers == {f for f in os.listdir(CSRC) if f.endswith(".h")}
        assert build._target(name, sources, header)[3] == os.path.join(build.OBJ, "flags_%s.txt" % name)
        assert not set(sources) & taken                                   # no source is shared with another row
        taken |= set(sources)
        includes = [len(re.findall(r'^#include "last_error\.h"', text[s + ".hip"], re.M)) for s in sources]
        assert sum(includes) == 1 and max(includes) == 1
        assert os.path.exists(lib)                                        # build() built it
    assert set(build.UDR_SOURCES) <= set(build.ALL_SOURCES)               # tools/isa_identity.py compares them


def test_call_raises_with_the_librarys_own_error_text():
    h = _udrlib.lib()
    assert h is _udrlib.lib()
    dummy = 1 << 20                                               # aligned non-NULL address, never dereferenced
    #        table  rows   N   D  S   ws     ranks  stream
    ranks = [dummy, dummy, 60, 3, 10, dummy, dummy, None]
    #     mean   logvar rows   N   D  S   ws     kl     stream
    kl = [dummy, dummy, dummy, 60, 3, 10, dummy, dummy, None]

    def put(good, i, v):
        return good[:i] + [v] + good[i + 1:]
    bad = [("dvae_udr_ranks", put(ranks, i, None)) for i in (0, 5, 6)] + [("dvae_udr_kl_dims", put(kl, i, None)) for i in (0, 1, 6, 7)]
    for name, good, sizes in (("dvae_udr_ranks", ranks, (2, 3, 4)), ("dvae_udr_kl_dims", kl, (3, 4, 5))):
        for i in sizes:
            bad += [(name, put(good, i, 0)), (name, put(good, i, -1))]
    bad.append(("dvae_udr_ranks", put(ranks, 3, _udrlib.MAX_D + 1)))
    bad.append(("dvae_udr_kl_dims", put(kl, 4, _udrlib.MAX_D + 1)))
    bad.append(("dvae_udr_ranks", put(ranks, 4, _udrlib.MAX_ROWS + 1)))                      # larger S is refused
    bad.append(("dvae_udr_ranks", put(put(ranks, 1, None), 2, _udrlib.MAX_ROWS + 1)))        # ... and all rows of a larger table
    for name, args in bad:
        with pytest.raises(_lib.DvaeHipError) as e:
            _udrlib.call(name, *args)
        own = h.dvae_udr_last_error().decode()
        assert "invalid argument" in own and "latent_ranks.hip" in own, (name, args, own)
        assert str(e.value) == "%s failed (-1): %s" % (name, own)
    assert "latent_ranks.hip" not in _unsuplib.lib().dvae_unsup_last_error().decode()       # every library keeps its own buffer
    # the workspace sizes: 0 out of range, one word or more in range, the ping-pong buffers above the one-workgroup path
    assert h.dvae_udr_ranks_ws_floats(60, 3, _udrlib.MAX_ROWS + 1) == 0 and h.dvae_udr_ranks_ws_floats(60, 65, 10) == 0
    assert h.dvae_udr_ranks_ws_floats(60, 3, 0) == h.dvae_udr_ranks_ws_floats(60, 3, 60) >= 1
    S = _udrlib.SMALL_ROWS + 1
    assert h.dvae_udr_ranks_ws_floats(60, 3, S) == 4 * 3 * S + 3 * 256 * 2 + 2 * 3 * 2
    assert h.dvae_udr_kl_dims_ws_floats(60, 3, 0) == 2 * 3 and h.dvae_udr_kl_dims_ws_floats(60, 3, _udrlib.KL_BLOCK_ROWS + 1) == 4 * 3
    assert h.dvae_udr_kl_dims_ws_floats(60, 0, 10) == 0


def test_source_obeys_the_rules_of_the_shared_plumbing():
    src = open(os.path.join(CSRC, "latent_ranks.hip")).read()
    assert not re.search(r"\bthread_local\b", src) and not re.search(r"^void set_error\(", src, re.M)
    for name in ("put_f64", "get_f64", "chunks_of", "lesser"):
        assert not re.search(r"^[ \w]*\b(?:void|double|int|T)\s+%s\s*\([^;{]*\)\s*\{" % name, src, re.M), name
    assert not re.search(r"\bbelow\s*\+=.*<=\s*x\b", src)
    assert '#include "table_stats.h"' in src
    assert not re.search(r"atomic\w*\s*\(\s*\(?\s*(float|double)", src) and "while" not in src      # no float atomics, no spinning


# ---- 2. the restatement against scipy / sklearn -------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.HARD + ("gauss",))
def test_reference_ranks_are_scipys(kind):
    stats = pytest.importorskip("scipy.stats")
    table = R.hard_table(kind, 301, 3)
    want = np.stack([stats.rankdata(table[:, d].astype(np.float64), method="average") for d in range(3)], axis=1)
    got = R.ranks(table)
    assert got.dtype == np.float64 and got.tobytes() == want.tobytes()
    rows = np.array([5, 5, 300, 0, 17, 5])                                 # repeats tie, order is the selection's
    want = np.stack([stats.rankdata(table[rows, d].astype(np.float64), method="average") for d in range(3)], axis=1)
    assert R.ranks(table, rows).tobytes() == want.tobytes()


def test_reference_spearman_is_scipys():
    stats = pytest.importorskip("scipy.stats")
    rng = np.random.default_rng(0)
    a = np.round(rng.standard_normal((400, 3)) * 3).astype(np.float32)     # with ties
    b = (a[:, [2, 0, 1]] ** 3 + rng.standard_normal((400, 3))).astype(np.float32)
    got = R.spearman(a, b, np.ones(3, bool), np.ones(3, bool))
    for i in range(3):
        for j in range(3):
            assert abs(got[i, j] - abs(stats.spearmanr(a[:, i], b[:, j])[0])) <= 1e-13
    masked = R.spearman(a, b, np.array([True, False, True]), np.ones(3, bool))
    assert not masked[1].any() and np.array_equal(masked[[0, 2]], got[[0, 2]])


def _lasso_case(S, Dx, Dy, alpha, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((S, Dx)) @ (np.eye(Dx) + 0.3 * rng.standard_normal((Dx, Dx)))
    y = x @ (rng.standard_normal((Dx, Dy)) * (rng.random((Dx, Dy)) < 0.5)) + rng.standard_normal((S, Dy))
    mask_x, mask_y = np.ones(Dx, bool), np.ones(Dy, bool)
    mask_x[Dx - 1] = False                                                 # a masked latent: a zero column
    x[:, 0] = 0.25 if seed == 2 else x[:, 0]                               # a constant one
    return x.astype(np.float32), y.astype(np.float32), mask_x, mask_y


def test_reference_lasso_is_sklearns():
    lm = pytest.importorskip("sklearn.linear_model")
    worst = 0.0
    for S, Dx, Dy, alpha, seed in LASSO_CASES:
        x, y, mx, my = _lasso_case(S, Dx, Dy, alpha, seed)
        model = lm.Lasso(alpha=alpha, tol=1e-12, max_iter=100000).fit(R.standardised(x, mx), R.standardised(y, my))
        want = np.abs(model.coef_).T                                       # [Dx, Dy], as udr.py transposes it
        got = R.lasso(x, y, mx, my, alpha)
        assert got.shape == want.shape == (Dx, Dy) and not got[Dx - 1].any()
        worst = max(worst, np.abs(got - want).max())
    print("worst |coefficient difference| to sklearn: %.3g" % worst)
    assert worst <= min(100 * LASSO_WORST, 1e-8)


# ---- 3. pair and model scores on hand-made matrices ---------------------------------------------------------------------------
@pytest.mark.parametrize("score", [R.pair_score, E.udr_pair_score], ids=["reference", "evaluate"])
def test_pair_score_of_known_matrices(score):
    for D in (1, 2, 5):
        perm = np.eye(D)[np.random.default_rng(D).permutation(D)]
        assert score(perm) == 1.0 and score(0.37 * perm) == pytest.approx(0.37, abs=1e-15)
        assert score(np.full((D, D), 0.4)) == pytest.approx(0.4 / D, abs=1e-15)
        assert score(np.ones((D, D))) == pytest.approx(1.0 / D, abs=1e-15)
    R3 = np.array([[1.0, 0, 0], [0, 0, 0], [0, 0, 0.5]])                   # a zero row and a zero column: 0 / 0 counts as 0
    assert score(R3) == pytest.approx(0.5 * ((1 + 0 + 0.5) / 3 + (1 + 0 + 0.5) / 3), abs=1e-15)
    assert score(np.zeros((3, 3))) == 0.0
    assert score(np.array([[0.6, 0.2]])) == pytest.approx(0.5 * ((0.6 + 0.2) / 2 + 0.36 / 0.8), abs=1e-15)   # not square
    for shape in ((0, 0), (0, 3), (3, 0)):                                  # empty masks: 0.0, where disentanglement_lib raises
        assert score(np.zeros(shape)) == 0.0


@pytest.mark.parametrize("scores", [R.model_scores, E.udr_model_scores], ids=["reference", "evaluate"])
def test_model_score_is_the_median_over_the_others(scores):
    P = np.array([[0.0, 0.9, 0.2, 0.5], [0.1, 0.0, 0.3, 0.7], [0.4, 0.8, 0.0, 0.6], [1.0, 0.35, 0.25, 0.0]])
    assert np.allclose(scores(P[:2, :2]), [0.1, 0.9], atol=0, rtol=0)                       # M = 2: the other one
    assert np.allclose(scores(P[:3, :3]), [0.25, 0.85, 0.25], atol=1e-15, rtol=0)           # M = 3: the mean of two
    assert np.allclose(scores(P), [0.4, 0.8, 0.25, 0.6], atol=0, rtol=0)                    # M = 4: the middle one of three
    assert np.allclose(scores(P + 7 * np.eye(4)), scores(P), atol=0, rtol=0)                # the diagonal takes no part


# ---- 4. evaluate.py's host half against the restatement -----------------------------------------------------------------------
def _cov_of_pair(tables):
    def cov(i, j):
        return np.cov(np.concatenate([tables[i], tables[j]], axis=1).astype(np.float64).T, ddof=1)
    return cov


@pytest.mark.parametrize("correlation", E.UDR_CORRELATIONS)
@pytest.mark.parametrize("kind,D", R.END_TO_END + [("collapsed", 3)])
def test_host_combination_against_the_restatement(kind, D, correlation):
    """udr_from_statistics on fp64 numpy.cov of the reference's own ranks / means is the restatement; and every row and column sum of
    the restricted R of the end-to-end cases is at least 0.1 -- the GPU tolerance of the scores rests on that."""
    means, logvars = R.sweep(kind, D)
    ref = R.udr(means, logvars, correlation)
    kl = np.stack([R.kl_dims(m, lv) for m, lv in zip(means, logvars)])
    tables = [R.ranks(m) for m in means] if correlation == "spearman" else list(means)
    got = E.udr_from_statistics(kl, _cov_of_pair(tables), correlation)
    assert set(got) | {"n_samples", "correlation"} == set(ref)
    assert np.array_equal(got["n_active"], ref["n_active"]) and np.array_equal(got["kl"], ref["kl"])
    assert np.abs(got["raw_correlations"] - ref["raw_correlations"]).max() <= 1e-10
    assert np.abs(got["pairwise_scores"] - ref["pairwise_scores"]).max() <= 1e-9
    assert np.abs(got["model_scores"] - ref["model_scores"]).max() <= 1e-9
    assert not np.diag(got["pairwise_scores"]).any() and not got["raw_correlations"][range(3), range(3)].any()
    mask = kl > 0.01
    if kind == "collapsed":
        assert ref["n_active"][2] == 0 and ref["model_scores"][2] == 0.0 and not ref["pairwise_scores"][2].any()
        return
    assert list(ref["n_active"]) == [D - 1 if D >= 3 else D] * 3
    for i in range(3):
        for j in range(3):
            if i != j:
                Rij = ref["raw_correlations"][i, j][np.ix_(mask[i], mask[j])]
                assert Rij.sum(axis=0).min() >= 0.1 and Rij.sum(axis=1).min() >= 0.1, (i, j)


@pytest.mark.parametrize("correlation", E.UDR_CORRELATIONS)
def test_aligned_models_outrank_a_rotated_one(correlation):
    for D in (2, 10):
        aligned, rotated = (R.udr(*R.sweep(kind, D), correlation=correlation) for kind in ("aligned", "rotated"))
        assert aligned["model_scores"].min() > 0.6
        assert rotated["model_scores"][1] < aligned["model_scores"][1] - 0.2        # model 1 is the rotated one
        assert rotated["pairwise_scores"][0, 2] == pytest.approx(aligned["pairwise_scores"][0, 2], abs=1e-12)


def test_lasso_from_gram_is_the_restatements_descent():
    for S, Dx, Dy, alpha, seed in LASSO_CASES:
        x, y, mx, my = _lasso_case(S, Dx, Dy, alpha, seed)
        xs, ys = R.standardised(x, mx), R.standardised(y, my)
        G, C = xs.T @ xs / S, xs.T @ ys / S
        for b in range(Dy):
            assert np.abs(E.lasso_from_gram(G, C[:, b], alpha) - R.lasso_gram(G, C[:, b], alpha)).max() <= 1e-12
        cov = np.cov(np.concatenate([x, y], axis=1).astype(np.float64).T, ddof=1) if Dx == Dy else None
        if cov is not None:                                                # the Pearson blocks ARE the Gram matrices
            assert np.abs(E.udr_lasso_from_cov(cov, mx, my, alpha) - R.lasso(x, y, mx, my, alpha)).max() <= 1e-11


# ---- 5. argument errors, before any library load ------------------------------------------------------------------------------
def test_every_argument_check_raises_before_a_library_load(monkeypatch):
    def boom():
        raise AssertionError("a library was loaded")
    monkeypatch.setattr(_udrlib, "lib", boom)
    monkeypatch.setattr(_unsuplib, "lib", boom)
    t = torch.zeros(50, 4)
    good = ([t, t + 1], [t, t])
    for means, logvars, kw, exc, text in [
            ([t], [t], {}, ValueError, "two or more"),
            ([t, t], [t], {}, ValueError, "one table per model"),
            ([t, torch.zeros(50, 5)], [t, t], {}, ValueError, "like the first"),
            ([t, t], [t, torch.zeros(49, 4)], {}, ValueError, "like the first"),
            ([torch.zeros(50), t], [t, t], {}, ValueError, r"\[N, D\] table"),
            ([torch.zeros(50, 33)] * 2, [torch.zeros(50, 33)] * 2, {}, ValueError, "between 1 and 32"),
            (*good, dict(correlation="pearson"), ValueError, "correlation must be"),
            (*good, dict(n_samples=0), ValueError, "n_samples"),
            (*good, dict(n_samples=51), ValueError, "n_samples"),
            (*good, dict(kl_threshold=-1.0), ValueError, "kl_threshold"),
            (*good, dict(kl_threshold=float("nan")), ValueError, "kl_threshold"),
            (*good, dict(lasso_alpha=-0.1), ValueError, "lasso_alpha"),
            (*good, dict(rows=[0, 50]), ValueError, "rows must hold"),
            (*good, dict(rows=[]), ValueError, "rows must hold"),
            ([t, t * float("nan")], [t, t], {}, ValueError, "NaN or an infinity"),
            ([t, t], [t, t + float("inf")], {}, ValueError, "NaN or an infinity"),
            (*good, {}, _lib.DvaeHipError, "needs the table on the GPU")]:
        with pytest.raises(exc, match=text):
            E.udr_from_tables(means, logvars, **kw)
    with pytest.raises(TypeError):
        E.udr_from_tables(*good, n_bins=20)


class _Loader:
    def __init__(self, n):
        self.dataset = list(range(n))

    def __iter__(self):
        raise AssertionError("the loader was walked")


def test_compute_udr_checks_before_it_encodes(monkeypatch):
    from disvae_amd.models.vae import init_specific_model
    monkeypatch.setattr(_udrlib, "lib", lambda: (_ for _ in ()).throw(AssertionError("a library was loaded")))
    models = [init_specific_model("Burgess", (1, 32, 32), 3) for _ in range(2)]
    ev = E.Evaluator(models[0], None, is_progress_bar=False)
    models[1].train()
    for others, kw, exc in (([], {}, ValueError), (models[1:], dict(correlation="kendall"), ValueError),
                            (models[1:], dict(n_samples=41), ValueError), (models[1:], dict(n_bins=3), TypeError)):
        with pytest.raises(exc):
            ev.compute_udr(_Loader(40), others, **kw)
    assert models[1].training
