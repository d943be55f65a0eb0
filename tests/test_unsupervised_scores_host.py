"""CPU: the host side of the label-free scores -- the sixth library's C-ABI (include/dvae_unsup_hip.h ==
disvae_amd/_unsuplib.py == the built libdvae_unsup_hip.so), the build, the fp64 restatement (tests/unsup_ref.py) on tables whose
scores are known, the host combination of evaluate.py against the restatement, the precondition of the GPU tests' bounds, and
the argument errors raised before any library call."""
import ctypes
import importlib
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import info_ref as I
import unsup_ref as R
from disvae_amd import _evallib, _infolib, _irslib, _lib, _scorelib, _unsuplib, Evaluator
from disvae_amd.evaluate import unsupervised_scores_from_statistics, unsupervised_scores_from_table
from disvae_amd.models.losses import get_loss_f
from disvae_amd.models.vae import init_specific_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dvae_unsup_hip.h")
KERNELS = ("k_unsup_moments_part", "k_unsup_moments_finish", "k_unsup_zero", "k_unsup_pair_hist")
HP = dict(rec_dist="bernoulli", reg_anneal=0, betaH_B=4, betaB_initC=0, betaB_finC=25, betaB_G=1000, factor_G=6.4,
          latent_dim=4, lr_disc=1e-4, btcvae_A=1, btcvae_B=6.4, btcvae_G=1)
SCORE_KEYS = ("gaussian_total_correlation", "gaussian_wasserstein_correlation", "gaussian_wasserstein_correlation_norm",
              "mutual_info_score", "mutual_information", "active_units", "variances", "live")


# ---- 1. the library -----------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _nm(path, *flags):
    nm = shutil.which("nm") or shutil.which("llvm-nm", path="/opt/rocm/llvm/bin")
    assert nm, "no nm on this machine"
    return subprocess.run([nm] + list(flags) + [path], capture_output=True, text=True, check=True).stdout


def test_header_ctypes_table_and_exports_agree():
    declared = sorted(set(re.findall(r"\b(dvae_unsup_[a-zA-Z0-9_]+)\s*\(", _header())))
    assert declared == sorted(_unsuplib.SIGNATURES) and len(declared) == 6
    exported = sorted(set(re.findall(r" T (dvae_\w+)", _nm(os.path.abspath(_unsuplib.LIB_PATH), "-D", "--defined-only"))))
    assert exported == declared
    kinds = {ctypes.c_void_p: "p", ctypes.c_int: "i", ctypes.c_long: "l"}
    for name, params in re.findall(r"\b(dvae_unsup_[a-zA-Z0-9_]+)\s*\(([^)]*)\)", _header()):
        got = []
        for prm in [x.strip() for x in params.split(",") if x.strip() != "void"]:
            got.append("p" if "*" in prm else ("l" if prm.startswith("long") else "i"))
        assert got == [kinds[t] for t in _unsuplib.SIGNATURES[name]], name
    macros = {k: int(v) for k, v in re.findall(r"#define (DVAE_UNSUP_\w+) (\d+)", _header())}
    mirrored = {"DVAE_UNSUP_VERSION": _unsuplib.VERSION, "DVAE_UNSUP_MAX_D": _unsuplib.MAX_D, "DVAE_UNSUP_MAX_BINS": _unsuplib.MAX_BINS,
                "DVAE_UNSUP_MOMENTS_BLOCK_ROWS": _unsuplib.MOMENTS_BLOCK_ROWS, "DVAE_UNSUP_HIST_BLOCK_ROWS": _unsuplib.HIST_BLOCK_ROWS,
                "DVAE_UNSUP_MAX_BLOCKS": _unsuplib.MAX_BLOCKS, "DVAE_UNSUP_MOMENTS_THREAD_SUMS": _unsuplib.MOMENTS_THREAD_SUMS,
                "DVAE_UNSUP_HIST_LDS_INTS": _unsuplib.HIST_LDS_INTS}
    assert macros == mirrored                                            # every macro of the header, none besides
    assert (_unsuplib.MAX_D, _unsuplib.MAX_BINS) == (64, 64)
    assert _unsuplib.HIST_LDS_INTS * 4 <= 64 * 1024                      # a tile of counters stays at or below 64 KB
    assert _unsuplib.HIST_LDS_INTS >= _unsuplib.MAX_BINS ** 2            # ... and holds one pair of the most bins
    assert _unsuplib.lib().dvae_unsup_version() == _unsuplib.VERSION == 1
    text = open(HEADER).read()                                           # the header says why two outputs are fp64
    assert "double* col_mean" in text and "double* cov" in text and "log-determinant" in text and "NEVER rounded to fp32" in text


def test_argument_errors_are_reported_before_any_launch():
    h = _unsuplib.lib()
    dummy = 1 << 20                                               # aligned non-NULL address, never dereferenced
    #      table  rows   N   D  S   ws     min    max    mean   cov    stream
    mom = [dummy, dummy, 60, 3, 10, dummy, dummy, dummy, dummy, dummy, None]
    #       table  rows   edges  N   D  S   bins ws    counts stream
    hist = [dummy, dummy, dummy, 60, 3, 10, 20, None, dummy, None]

    def put(good, i, v):
        return good[:i] + [v] + good[i + 1:]
    bad = []
    for name, good, ptrs, sizes in (("dvae_unsup_moments", mom, (0, 5, 6, 7, 8, 9), (2, 3, 4)),
                                    ("dvae_unsup_pair_hist", hist, (0, 2, 8), (3, 4, 5, 6))):
        for i in ptrs:
            bad.append((name, put(good, i, None)))
        for i in sizes:
            bad += [(name, put(good, i, 0)), (name, put(good, i, -1))]
    bad.append(("dvae_unsup_moments", put(mom, 3, _unsuplib.MAX_D + 1)))                     # the limits
    bad.append(("dvae_unsup_pair_hist", put(hist, 4, _unsuplib.MAX_D + 1)))
    bad.append(("dvae_unsup_pair_hist", put(hist, 6, _unsuplib.MAX_BINS + 1)))
    bad.append(("dvae_unsup_pair_hist", put(hist, 4, 1)))                                    # one latent: no pair
    for name, good, n_at, s_at in (("dvae_unsup_moments", mom, 2, 4), ("dvae_unsup_pair_hist", hist, 3, 5)):
        bad.append((name, put(good, s_at, 1 << 31)))                                         # a count could pass 2^31 - 1
        bad.append((name, put(put(good, 1, None), n_at, 1 << 31)))                           # ... all N rows of too long a table
    for name, args in bad:
        with pytest.raises(_lib.DvaeHipError, match="invalid argument"):
            _unsuplib.call(name, *args)
        assert b"invalid argument" in h.dvae_unsup_last_error()
    for name, good, d_at in (("dvae_unsup_moments", mom, 3), ("dvae_unsup_pair_hist", hist, 4)):
        with pytest.raises(_lib.DvaeHipError, match="DVAE_UNSUP_MAX_D"):
            _unsuplib.call(name, *put(good, d_at, 65))
    with pytest.raises(_lib.DvaeHipError, match="DVAE_UNSUP_MAX_BINS"):
        _unsuplib.call("dvae_unsup_pair_hist", *put(hist, 6, 65))


def test_workspace_sizes_are_what_the_header_promises():
    h = _unsuplib.lib()
    ws = h.dvae_unsup_moments_ws_floats
    for N, D, S in ((0, 10, 4), (5, 0, 4), (-1, 10, 4), (5, -3, 4), (5, _unsuplib.MAX_D + 1, 4), (1 << 31, 10, 4), (5, 10, 1 << 31)):
        assert ws(N, D, S) == 0
    # one record per chunk: D (D + 3) / 2 doubles (the sums of x_d and of x_d x_e, d <= e) and 2 D floats (min, max); S <= 0: all N
    rec = 2 * (10 * 13 // 2) + 2 * 10
    assert ws(737280, 10, 0) == ws(737280, 10, 737280) == (737280 // _unsuplib.MOMENTS_BLOCK_ROWS) * rec
    assert ws(60, 10, 1) == rec and ws(60, 10, _unsuplib.MOMENTS_BLOCK_ROWS + 1) == 2 * rec
    assert ws(60, 10, 1 << 30) == _unsuplib.MAX_BLOCKS * rec
    assert ws(60, 64, 60) == 2 * (64 * 67 // 2) + 2 * 64
    assert h.dvae_unsup_pair_hist_ws_floats(737280, 10, 737280, 20) == 0


# ---- 2. the build -------------------------------------------------------------------------------------------------------------
def test_build_leaves_six_libraries_and_keeps_them_apart():
    g = importlib.import_module("__graft_entry__")
    g.build()
    paths = [os.path.abspath(m.LIB_PATH) for m in (_lib, _evallib, _scorelib, _infolib, _irslib, _unsuplib)]
    main, unsup = paths[0], paths[-1]
    assert os.path.dirname(main) == os.path.dirname(unsup) and os.path.basename(unsup) == "libdvae_unsup_hip.so"
    assert all(os.path.exists(p) for p in paths) and len(set(paths)) == 6
    spec = importlib.util.spec_from_file_location("dvae_build_unsup", os.path.join(ROOT, "disentangling-vae_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.UNSUP_SOURCES == ["latent_pairs"]
    assert not set(mod.UNSUP_SOURCES) & set(mod.SOURCES + mod.EVAL_SOURCES + mod.SCORE_SOURCES + mod.INFO_SOURCES + mod.IRS_SOURCES)
    assert os.path.abspath(mod.UNSUP_LIB) == unsup and any(h.endswith("dvae_unsup_hip.h") for h in mod.UNSUP_HEADERS)
    assert os.path.abspath(mod.build(verbose=False)) == main      # still the training library's path
    assert open(os.path.join(mod.OBJ, "flags_unsup.txt")).read() == " ".join(mod.FLAGS + mod.UNSUP_SOURCES)
    others = [_nm(p, "-C") for p in paths[:-1]]
    in_unsup = _nm(unsup, "-C")
    for k in KERNELS:
        assert all(not re.search(r"\b%s\b" % k, text) for text in others), k
        assert re.search(r"__device_stub__%s\b" % k, in_unsup), k + " is not in libdvae_unsup_hip.so"
    assert all("dvae_unsup_" not in text and "k_unsup_" not in text for text in others)
    assert not any(s in in_unsup for s in ("dvae_score_", "dvae_eval_", "dvae_info_", "dvae_irs_", "k_info_", "k_irs_"))


# ---- 3. the restatement -------------------------------------------------------------------------------------------------------
def test_wasserstein_eigenvalue_form_is_scipys_matrix_square_root():
    """2 tr C - 2 tr sqrtm(diag(v) C): diag(v) C = V^1/2 (V^1/2 C V^1/2) V^-1/2 is similar to a symmetric PSD matrix, so the trace
    of its square root is the sum of the square roots of that matrix's eigenvalues."""
    linalg = pytest.importorskip("scipy").linalg
    rng = np.random.default_rng(5)
    for D in (1, 2, 3, 10, 17):
        a = rng.standard_normal((4 * D + 2, D)) * rng.uniform(0.1, 3.0, size=D)
        a[:, -1] += 0.7 * a[:, 0]
        C = np.atleast_2d(np.cov(a.T, ddof=1))
        want = 2 * np.trace(C) - 2 * np.trace(linalg.sqrtm(np.diag(np.diag(C)) @ C)).real
        live = np.ones(D, dtype=bool)
        _tc, got, norm = R.gaussian_scores(C, live)
        assert abs(got - want) <= 1e-10 * max(1.0, np.trace(C)) and abs(norm - want / np.trace(C)) <= 1e-10
        mine = unsupervised_scores_from_statistics(np.zeros(D), np.ones(D), C, np.zeros((D * (D - 1) // 2, 1, 1)) + 9, 1)
        assert abs(mine["gaussian_wasserstein_correlation"] - want) <= 1e-10 * max(1.0, np.trace(C))


# gauss on (3, 4, 5), D = 3: total correlation 0.0387084 and Wasserstein correlation 0.0254804 to six digits
KNOWN_GAUSS = (0.038708424547319265, 0.025480411105377243)


def test_reference_scores_of_known_tables():
    """ideal_table: K independent factor columns of a product grid and D - K constants -- every score exactly 0.  rotated_table on
    (2, 3, 6, 20), D = 7: columns 0 and 1 are (a + b) / sqrt 2 and (a - b) / sqrt 2 of two independent standardised factors; their
    covariance stays the identity, so by the definition (numpy.cov, slogdet on the live block) the total correlation is 0 to
    rounding -- finite, NOT inf -- while their discretised mutual information is large.  The singular case that does give inf is
    a live column repeated."""
    for lat, D in (((3, 4, 5), 5), ((2, 3, 6, 20), 7)):
        s = R.scores(I.ideal_table(lat, D))
        assert s["gaussian_total_correlation"] == 0.0 and s["gaussian_wasserstein_correlation"] == 0.0
        assert s["gaussian_wasserstein_correlation_norm"] == 0.0 and s["mutual_info_score"] == 0.0
        assert s["live"].sum() == len(lat) and list(s["live"]) == [True] * len(lat) + [False] * (D - len(lat))
    s = R.scores(I.make_table((3, 4, 5), 3, "gauss"))
    for got, want in zip((s["gaussian_total_correlation"], s["gaussian_wasserstein_correlation"]), KNOWN_GAUSS):
        assert abs(got - want) <= 1e-12
    assert round(KNOWN_GAUSS[0], 7) == 0.0387084 and round(KNOWN_GAUSS[1], 7) == 0.0254804
    s = R.scores(I.rotated_table((2, 3, 6, 20), 7))
    print("rotated (2, 3, 6, 20), D = 7: TC %r, MI[0, 1] %.4f" % (s["gaussian_total_correlation"], s["mutual_information"][0, 1]))
    assert abs(s["gaussian_total_correlation"]) <= 1e-12 and s["mutual_information"][0, 1] > 0.5 and s["live"].sum() == 4
    twice = I.make_table((3, 4, 5), 2, "gauss")
    twice[:, 1] = twice[:, 0]
    assert R.scores(twice)["gaussian_total_correlation"] == np.inf
    const = R.scores(I.make_table((3, 4, 5), 4, "const"))
    assert not const["live"].any() and const["gaussian_total_correlation"] == 0.0 and const["mutual_info_score"] == 0.0


# ---- 4. the host combination --------------------------------------------------------------------------------------------------
def _assert_equal_scores(got, ref, what):
    assert set(got) == set(SCORE_KEYS) and set(ref) == set(SCORE_KEYS) | {"n_samples", "n_bins"}, what
    for key in SCORE_KEYS:
        if key in ("live", "active_units"):
            assert np.array_equal(got[key], ref[key]), (what, key)
        elif np.isscalar(ref[key]) and np.isinf(ref[key]):
            assert got[key] == ref[key], (what, key)
        else:
            np.testing.assert_allclose(got[key], ref[key], rtol=0, atol=1e-12, err_msg="%s %s" % (what, key))


def test_host_combination_is_the_restatement():
    cases = [(R.end_to_end_case(*c), c[3], str(c)) for c in R.END_TO_END]
    middle = I.make_table((3, 4, 5), 5, "gauss")
    middle[:, 2] = np.float32(-0.75)                               # a constant column in the middle
    twice = I.make_table((3, 4, 5), 2, "gauss")
    twice[:, 1] = twice[:, 0]                                      # a singular live block: inf
    cases += [((middle, None), 20, "constant column in the middle"), ((I.make_table((60,), 1, "gauss"), None), 20, "D = 1"),
              ((I.make_table((60,), 2, "offset"), None), 7, "D = 2"), ((I.make_table((60,), 3, "gauss"), np.array([7])), 20, "S = 1"),
              ((twice, None), 20, "a repeated column")]
    for (table, rows), n_bins, what in cases:
        ref = R.scores(table, n_bins, rows)
        mom = R.moments(table, rows)
        counts, _ = R.pair_counts(table, n_bins, rows)
        got = unsupervised_scores_from_statistics(mom["min"], mom["max"], mom["cov"], counts if table.shape[1] > 1 else None, n_bins)
        _assert_equal_scores(got, ref, what)
        assert isinstance(got["gaussian_total_correlation"], float) and isinstance(got["active_units"], int)
        assert got["live"].dtype == bool and np.array_equal(got["mutual_information"], got["mutual_information"].T)
        assert not np.diag(got["mutual_information"]).any()
    assert got["gaussian_total_correlation"] == np.inf
    low = unsupervised_scores_from_statistics(mom["min"], mom["max"], mom["cov"], counts, 20, active_threshold=1e9)
    assert low["active_units"] == 0


# ---- 5. the precondition of the GPU tests' bounds -------------------------------------------------------------------------------
def test_chunked_fp64_sums_stay_within_a_quarter_of_the_covariance_bound():
    """For every moments case of tests/test_gpu_unsupervised_scores.py the first-row-shifted sums taken in fp64 in chunks of 1024
    rows stay within a quarter of the tolerance of unsup_ref (worst 0.018: gauss, D = 17, S = 63), so the bound tests the kernel's
    accumulation and not the formula."""
    worst = 0.0
    for c in R.CASES + R.switch_cases(_unsuplib):
        k = R.case(*c)
        mom = k["moments"]
        mean, cov = R.chunked_moments(k["table"], k["rows"], chunk=1024)
        ratio = max(R.worst_ratio(cov, mom["cov"], R.cov_tolerance(mom)), R.worst_ratio(mean, mom["mean"], R.mean_tolerance(mom)))
        worst = max(worst, ratio)
        assert ratio <= 0.25, (c, ratio)
    print("worst chunked-fp64 error / tolerance %.4f" % worst)


def test_end_to_end_tables_are_well_conditioned():
    """cond(correlation matrix of the live block) <= 1e3 on every end-to-end table (worst 10.7: ties, D = 17), so the first-order
    bound of the Gaussian scores holds with room."""
    worst = 0.0
    for c in R.END_TO_END:
        table, rows = R.end_to_end_case(*c)
        corr, live = R.live_correlation(R.moments(table, rows))
        if live.any():
            worst = max(worst, np.linalg.cond(corr))
            assert np.linalg.cond(corr) <= 1e3, c
    print("worst condition number %.1f" % worst)
    assert any(R.END_TO_END[i][0] == "mixed" for i in range(len(R.END_TO_END)))
    kinds = {c[0] for c in R.END_TO_END}
    assert {"gauss", "offset", "ties", "const", "disent", "mixed"} <= kinds


# ---- 6. errors before any library call ----------------------------------------------------------------------------------------
class _NoFactors:
    """a data set WITHOUT lat_sizes / lat_names: what CelebA, Chairs and MNIST look like"""

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


class _Loader:
    def __init__(self, dataset, batches):
        self.dataset, self.batches = dataset, batches

    def __iter__(self):
        if self.batches is None:
            raise AssertionError("iterated before the arguments were checked")
        return iter(self.batches)


def test_argument_errors_raise_before_any_library_call(monkeypatch):
    def no_library():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_unsuplib, "lib", no_library)
    table = torch.zeros(6, 4)
    for kw, msg in ((dict(n_bins=0), r"n_bins must lie in \[1, 64\]"), (dict(n_bins=65), r"n_bins must lie in \[1, 64\]"),
                    (dict(n_samples=7), r"n_samples must lie in \[1, 6\]"), (dict(n_samples=0), "n_samples must be at least 1"),
                    (dict(rows=[0, 6]), r"in \[0, 6\)"), (dict(rows=[-1]), r"in \[0, 6\)"), (dict(rows=[]), "one row number or more")):
        with pytest.raises(ValueError, match=msg):
            unsupervised_scores_from_table(table, **kw)
    with pytest.raises(ValueError, match="table"):
        unsupervised_scores_from_table(torch.zeros(6))
    with pytest.raises(ValueError, match="between 1 and 64"):
        unsupervised_scores_from_table(torch.zeros(6, 65))
    with pytest.raises(ValueError, match="between 1 and 64"):
        unsupervised_scores_from_table(torch.zeros(6, 0))
    with pytest.raises(ValueError, match="one row or more"):
        unsupervised_scores_from_table(torch.zeros(0, 4))
    bad = table.clone()
    bad[4, 1] = float("nan")
    with pytest.raises(ValueError, match="NaN"):
        unsupervised_scores_from_table(bad)
    with pytest.raises(_lib.DvaeHipError, match="no CPU"):
        unsupervised_scores_from_table(table)
    model = init_specific_model("Burgess", (1, 32, 32), 4)              # on the CPU: any device work would raise DvaeHipError
    ev = Evaluator(model, get_loss_f("VAE", **HP), device=torch.device("cpu"), is_progress_bar=False)
    for kw, msg in ((dict(n_bins=0), "n_bins must lie"), (dict(n_bins=100), "n_bins must lie"), (dict(n_samples=7), "n_samples must lie"),
                    (dict(n_samples=-2), "n_samples must be at least 1")):
        with pytest.raises(ValueError, match=msg):
            ev.compute_unsupervised_scores(_Loader(_NoFactors(6), None), **kw)
    model.train()
    loader = _Loader(_NoFactors(6), [(torch.rand(4, 1, 32, 32), None), (torch.rand(2, 1, 32, 32), None)])
    assert not hasattr(loader.dataset, "lat_sizes")
    with pytest.raises(_lib.DvaeHipError):                              # no demand for lat_sizes: the native encoder refuses the CPU
        ev.compute_unsupervised_scores(loader)
    assert model.training                                               # ... and the mode is as it was
    model.eval()
    with pytest.raises(_lib.DvaeHipError):
        ev.compute_unsupervised_scores(loader)
    assert not model.training
