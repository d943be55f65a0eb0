"""CPU: the host side of the FactorVAE / beta-VAE scores -- the third library's C-ABI (include/dvae_score_hip.h ==
disvae_amd/_scorelib.py == the built libdvae_score_hip.so), the build, the row drawing, the classifier, the fp64 restatement
(tests/scores_ref.py) on tables whose scores are known, and the argument errors Evaluator.compute_factor_scores raises before
any device work."""
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

import scores_ref as R
from disvae_amd import _evallib, _lib, _scorelib, Evaluator
from disvae_amd.evaluate import draw_fixed_factor_rows, factor_scores_from_table, fit_logistic_regression
from disvae_amd.models.losses import get_loss_f
from disvae_amd.models.vae import init_specific_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dvae_score_hip.h")
KERNELS = ("k_group_var", "k_pair_absdiff", "k_vote_argmin", "k_vote_count_lds", "k_vote_count_wide")
HP = dict(rec_dist="bernoulli", reg_anneal=0, betaH_B=4, betaB_initC=0, betaB_finC=25, betaB_G=1000, factor_G=6.4,
          latent_dim=4, lr_disc=1e-4, btcvae_A=1, btcvae_B=6.4, btcvae_G=1)


# ---- 1. the library -----------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _nm(path, *flags):
    nm = shutil.which("nm") or shutil.which("llvm-nm", path="/opt/rocm/llvm/bin")
    assert nm, "no nm on this machine"
    return subprocess.run([nm] + list(flags) + [path], capture_output=True, text=True, check=True).stdout


def test_header_ctypes_table_and_exports_agree():
    declared = sorted(set(re.findall(r"\b(dvae_score_[a-zA-Z0-9_]+)\s*\(", _header())))
    assert declared == sorted(_scorelib.SIGNATURES) and len(declared) == 6
    exported = sorted(set(re.findall(r" T (dvae_\w+)", _nm(os.path.abspath(_scorelib.LIB_PATH), "-D", "--defined-only"))))
    assert exported == declared
    kinds = {ctypes.c_void_p: "p", ctypes.c_int: "i", ctypes.c_long: "l"}
    for name, params in re.findall(r"\b(dvae_score_[a-zA-Z0-9_]+)\s*\(([^)]*)\)", _header()):
        got = []
        for prm in [x.strip() for x in params.split(",") if x.strip() != "void"]:
            got.append("p" if "*" in prm else ("l" if prm.startswith("long") else "i"))
        assert got == [kinds[t] for t in _scorelib.SIGNATURES[name]], name
    macros = dict(re.findall(r"#define (DVAE_SCORE_\w+) (\d+)", _header()))
    assert int(macros["DVAE_SCORE_VERSION"]) == _scorelib.VERSION == 1 == _scorelib.lib().dvae_score_version()
    assert int(macros["DVAE_SCORE_WAVE_MAX_L"]) == _scorelib.WAVE_MAX_L
    assert int(macros["DVAE_SCORE_VOTE_LDS_BINS"]) == _scorelib.VOTE_LDS_BINS


def test_argument_errors_are_reported_before_any_launch():
    h = _scorelib.lib()
    dummy = 1 << 20                                               # aligned non-NULL address, never dereferenced
    var = [dummy, dummy, 50, 3, 4, 5, dummy, dummy, dummy, None]  # (inv_scale and ws may be NULL)
    diff = [dummy, dummy, dummy, 50, 3, 4, 5, dummy, None]
    vote = [dummy, dummy, dummy, 4, 3, 2, dummy, dummy, None]
    bad = []
    for name, good, ptrs, sizes in (("dvae_score_group_var", var, (0, 1, 8), (2, 3, 4, 5)),
                                    ("dvae_score_pair_absdiff", diff, (0, 1, 2, 7), (3, 4, 5, 6)),
                                    ("dvae_score_vote", vote, (0, 1, 2, 6, 7), (3, 4, 5))):
        for i in ptrs:
            bad.append((name, good[:i] + [None] + good[i + 1:]))
        for i in sizes:
            bad.append((name, good[:i] + [0] + good[i + 1:]))
            bad.append((name, good[:i] + [-1] + good[i + 1:]))
    bad.append(("dvae_score_group_var", var[:5] + [1] + var[6:]))  # a variance needs two rows
    for name, args in bad:
        with pytest.raises(_lib.DvaeHipError, match="invalid argument"):
            _scorelib.call(name, *args)
        assert b"invalid argument" in h.dvae_score_last_error()
    ws = h.dvae_score_group_var_ws_floats
    for N, D, V, L in ((0, 10, 5, 4), (5, 0, 5, 4), (5, 10, 0, 4), (5, 10, 5, 0), (-1, 10, 5, 4), (5, -3, 5, 4), (5, 10, -7, 4),
                       (5, 10, 5, -2)):
        assert ws(N, D, V, L) == 0


# ---- 2. the build -------------------------------------------------------------------------------------------------------------
def test_build_leaves_three_libraries_and_keeps_them_apart():
    g = importlib.import_module("__graft_entry__")
    g.build()
    main, ev, sc = (os.path.abspath(m.LIB_PATH) for m in (_lib, _evallib, _scorelib))
    assert os.path.dirname(main) == os.path.dirname(ev) == os.path.dirname(sc)
    assert all(os.path.exists(p) for p in (main, ev, sc)) and os.path.basename(sc) == "libdvae_score_hip.so"
    spec = importlib.util.spec_from_file_location("dvae_build_scores", os.path.join(ROOT, "disentangling-vae_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.SCORE_SOURCES == ["factor_scores"] and mod.EVAL_SOURCES == ["elbo_decomp"] and "factor_scores" not in mod.SOURCES
    assert os.path.abspath(mod.SCORE_LIB) == sc and any(h.endswith("dvae_score_hip.h") for h in mod.SCORE_HEADERS)
    assert os.path.abspath(mod.build(verbose=False)) == main      # still the training library's path
    in_main, in_eval, in_score = _nm(main, "-C"), _nm(ev, "-C"), _nm(sc, "-C")
    for k in KERNELS:
        assert not re.search(r"\b%s\b" % k, in_main) and not re.search(r"\b%s\b" % k, in_eval), k
        assert re.search(r"__device_stub__%s\b" % k, in_score), k + " is not in libdvae_score_hip.so"
    assert "dvae_score_" not in in_main and "dvae_score_" not in in_eval
    assert "dvae_eval_" not in in_score
    assert _lib.lib().dvae_version() == 109 and _evallib.lib().dvae_eval_version() == 1


# ---- 3. the row drawing -------------------------------------------------------------------------------------------------------
def test_draw_fixed_factor_rows():
    sizes, V, L = [3, 1, 4, 5], 300, 16
    N = int(np.prod(sizes))
    values = R.factor_values(sizes)                                          # [N, K]
    state = torch.get_rng_state()

    def draw(seed, paired):
        return draw_fixed_factor_rows(sizes, V, L, torch.Generator().manual_seed(seed), device="cpu", paired=paired)
    factor, rows = draw(0, False)
    assert factor.dtype == torch.int32 and rows.dtype == torch.int64 and rows.shape == (V, L) and rows.is_contiguous()
    assert 0 <= int(rows.min()) and int(rows.max()) < N
    assert set(factor.tolist()) == {0, 2, 3}                                 # factor 1 has one value: never drawn
    vals = values[rows.numpy()]                                              # [V, L, K]
    fixed = np.take_along_axis(vals, factor.numpy().astype(np.int64)[:, None, None].repeat(L, 1), axis=2)[:, :, 0]
    assert (fixed == fixed[:, :1]).all()                                     # constant within the group
    for k in (0, 2, 3):
        assert len(np.unique(fixed[factor.numpy() == k])) == sizes[k]         # ... and every value of it occurs
        others = vals[factor.numpy() != k][:, :, k]
        assert (others.min(axis=1) != others.max(axis=1)).any(), k           # free factors vary inside a group
    factor2, rows_a, rows_b = draw(0, True)
    assert rows_a.shape == rows_b.shape == (V, L) and 0 <= int(min(rows_a.min(), rows_b.min()))
    assert int(max(rows_a.max(), rows_b.max())) < N and set(factor2.tolist()) == {0, 2, 3}
    va, vb = values[rows_a.numpy()], values[rows_b.numpy()]
    idx = factor2.numpy().astype(np.int64)[:, None, None].repeat(L, 1)
    fa, fb = np.take_along_axis(va, idx, axis=2)[:, :, 0], np.take_along_axis(vb, idx, axis=2)[:, :, 0]
    assert (fa == fb).all()                                                  # each pair shares the value ...
    assert (fa.min(axis=1) != fa.max(axis=1)).any()                          # ... which differs from pair to pair
    assert not (rows_a == rows_b).all()
    for k in (0, 2, 3):
        sel = factor2.numpy() != k
        assert (va[sel][:, :, k] != vb[sel][:, :, k]).any(), k               # the other factors are independent on both sides
    again = draw(0, False)
    assert torch.equal(again[0], factor) and torch.equal(again[1], rows)
    other = draw(1, False)
    assert not torch.equal(other[1], rows)
    assert torch.equal(torch.get_rng_state(), state)                         # the global generator is untouched
    with pytest.raises(ValueError, match="two values"):
        draw_fixed_factor_rows([1, 1], 4, 4, torch.Generator().manual_seed(0))


# ---- 4. the restatement and the classifier -----------------------------------------------------------------------------------
@pytest.mark.parametrize("lat_sizes", [(3, 4, 5, 6), (3, 6, 40, 32, 32)])
def test_reference_scores_of_ideal_and_rotated_tables(lat_sizes):
    K = len(lat_sizes)
    draws = R.make_draws(lat_sizes, 2000, 1000, 64, 10000, seed=1)
    ideal, _ = R.scores(R.synthetic_table(lat_sizes, "ideal"), lat_sizes, draws)
    rotated, det = R.scores(R.synthetic_table(lat_sizes, "rotated"), lat_sizes, draws)
    print(lat_sizes, ideal, rotated)
    assert R.synthetic_table(lat_sizes, "ideal").shape == (int(np.prod(lat_sizes)), K + 2)
    for k in ("factor_vae_train", "factor_vae_eval", "beta_vae_train", "beta_vae_eval"):
        assert ideal[k] == 1.0, (k, ideal[k])
    assert ideal["n_active"] == K and rotated["n_active"] == K
    assert rotated["factor_vae_train"] < 1.0 and rotated["factor_vae_eval"] < 1.0
    assert 1.0 / K < rotated["factor_vae_eval"] and 1.0 / K < rotated["beta_vae_eval"] <= 1.0
    assert (ideal["n_train"], ideal["n_eval"], ideal["batch_size"]) == (2000, 1000, 64)
    # the restatement's own classifier sits at the optimum of the objective
    y = np.searchsorted(det["classes"], det["labels_train"])
    _, dW, db, _ = R.logreg_loss_grad(det["W"], det["b"], det["features_train"], y)
    assert max(np.abs(dW).max(), np.abs(db).max()) < 1e-8


def test_classifier_reaches_the_optimum_on_the_rotated_features():
    lat_sizes = (3, 4, 5, 6)
    _, det = R.scores(R.synthetic_table(lat_sizes, "rotated"), lat_sizes, R.make_draws(lat_sizes, 2000, 1000, 64, 10000, seed=1))
    y = np.searchsorted(det["classes"], det["labels_train"])
    W, b = fit_logistic_regression(det["features_train"], y, len(det["classes"]))
    assert W.dtype == b.dtype == torch.float64 and W.shape == (4, 6) and b.shape == (4,)
    _, dW, db, _ = R.logreg_loss_grad(W.numpy(), b.numpy(), det["features_train"], y)
    worst = max(np.abs(dW).max(), np.abs(db).max())
    print("largest gradient entry at the returned (W, b): %.3e" % worst)
    assert worst < 1e-6
    # strictly convex in W: the independent Newton fit of the restatement lands on the same weights and the same decisions
    np.testing.assert_allclose(W.numpy(), det["W"], atol=1e-3 * np.abs(det["W"]).max())
    assert R.accuracy(W.numpy(), b.numpy(), det["classes"], det["features_eval"], det["labels_eval"]) == \
        R.accuracy(det["W"], det["b"], det["classes"], det["features_eval"], det["labels_eval"])


def test_reference_vote_rules():
    stat = np.array([[3.0, 1.0, 1.0, 0.5], [np.nan, 2.0, 2.0, 9.0], [np.nan, np.nan, np.nan, 0.0]])
    argmin, votes = R.vote(stat, np.array([0, 1, 1]), np.array([1, 1, 1, 0]), 2)
    assert argmin.tolist() == [1, 1, -1] and votes.tolist() == [[0, 1, 0, 0], [0, 1, 0, 0]]
    assert R.vote(stat, np.array([0, 1, 1]), np.zeros(4, dtype=int), 2)[0].tolist() == [-1, -1, -1]
    assert R.near_ties(np.array([[1.0, 1.00001, 5.0], [1.0, 2.0, np.nan], [1.0, 1.0, 1.0]]), [1, 1, 1]).tolist() == [True, False, True]
    assert R.near_ties(np.array([[1.0, 1.00001, 5.0]]), [1, 0, 1]).tolist() == [False]


# ---- 5. errors before any device work -----------------------------------------------------------------------------------------
class _Factors:
    lat_sizes = np.array([3, 2])
    lat_names = ("a", "b")

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


class _Loader:
    def __init__(self, dataset, batches):
        self.dataset, self.batches = dataset, batches

    def __iter__(self):
        if self.batches is None:
            raise AssertionError("iterated before the sizes were checked")
        return iter(self.batches)


def test_evaluator_argument_errors():
    model = init_specific_model("Burgess", (1, 32, 32), 4)              # on the CPU: any device work would raise DvaeHipError
    ev = Evaluator(model, get_loss_f("VAE", **HP), device=torch.device("cpu"), is_progress_bar=False)
    with pytest.raises(ValueError, match="known true factors"):
        ev.compute_factor_scores(_Loader([0, 1, 2], None))
    sized = _Loader(_Factors(6), None)
    for kw, msg in ((dict(n_train=0), "n_train and n_eval must be >= 1"), (dict(n_eval=-1), "n_train and n_eval must be >= 1"),
                    (dict(batch_size=1), "batch_size must be >= 2"), (dict(n_variance=1), "two rows or more")):
        with pytest.raises(ValueError, match=msg):
            ev.compute_factor_scores(sized, **kw)
    with pytest.raises(ValueError, match=r"data set of 5 images does not enumerate lat_sizes=\[3, 2\]"):
        ev.compute_factor_scores(_Loader(_Factors(5), None))
    model.train()
    loader = _Loader(_Factors(6), [(torch.rand(4, 1, 32, 32), None), (torch.rand(2, 1, 32, 32), None)])
    with pytest.raises(_lib.DvaeHipError):                              # valid arguments: the native encoder refuses the CPU
        ev.compute_factor_scores(loader, n_train=4, n_eval=4, batch_size=2)
    assert model.training                                               # ... and the mode is as it was
    # the table-level function: the same size checks, then no CPU fallback
    table = torch.zeros(6, 4)
    with pytest.raises(ValueError, match="does not enumerate"):
        factor_scores_from_table(table, [3, 3])
    with pytest.raises(ValueError, match="batch_size must be >= 2"):
        factor_scores_from_table(table, [3, 2], batch_size=1)
    with pytest.raises(ValueError, match="two values"):
        factor_scores_from_table(torch.zeros(1, 4), [1, 1])
    with pytest.raises(_lib.DvaeHipError, match="no CPU"):
        factor_scores_from_table(table, [3, 2], n_train=4, n_eval=4, batch_size=2)
