"""GPU: the unsupervised disentanglement ranking -- the kernels of csrc/latent_ranks.hip (libdvae_udr_hip.so) and udr_from_tables /
Evaluator.compute_udr on top of them against the fp64 numpy restatement tests/udr_ref.py, whose docstring derives every
tolerance used here.  The ranks are EXACT: every comparison of them is a comparison of bytes.
Measured on the MI355X, worst error / tolerance over all cases below: KL per dimension 0.0045, R 0.0006 (both correlations), pair
scores below 0.0001."""
import json
import logging
import os

import numpy as np
import pytest
import torch

import latent_regimes as LR
import udr_ref as R
from gpu_util import DEV, dev, keep, stream
from guard_util import Guarded, run_contract
from disvae_amd import _lib, _udrlib, _unsuplib, Evaluator
from disvae_amd.evaluate import udr_from_tables
from disvae_amd.models.losses import get_loss_f
from disvae_amd.models.vae import init_specific_model

pytestmark = pytest.mark.gpu

KEYS = {"model_scores", "pairwise_scores", "raw_correlations", "kl", "n_active", "n_samples", "correlation"}
NAN_A, NAN_B = 0x7FC5A5A5, 0xFFE1B00B                               # what the workspace holds before a call: two NaN patterns


def _rows(rows):
    return None if rows is None else keep(torch.from_numpy(np.asarray(rows, dtype=np.int64)).to(DEV))


def run_ranks(table, rows=None, fill=NAN_A):
    N, D = table.shape
    S = N if rows is None else len(rows)
    t, r = dev(torch.from_numpy(table)), _rows(rows)
    need = _udrlib.lib().dvae_udr_ranks_ws_floats(N, D, S)
    assert need >= 1
    ws = keep(torch.full((need,), fill - (1 << 32) if fill >= 1 << 31 else fill, dtype=torch.int32, device=DEV))
    out = torch.full((S, D), float("nan"), device=DEV)
    _udrlib.call("dvae_udr_ranks", t.data_ptr(), None if r is None else r.data_ptr(), N, D, S, ws.data_ptr(), out.data_ptr(), stream())
    return out.cpu().numpy()


def run_kl(mean, logvar, rows=None):
    N, D = mean.shape
    S = N if rows is None else len(rows)
    m, lv, r = dev(torch.from_numpy(mean)), dev(torch.from_numpy(logvar)), _rows(rows)
    need = _udrlib.lib().dvae_udr_kl_dims_ws_floats(N, D, S)
    assert need >= 2 * D
    ws = keep(torch.full((need,), float("nan"), device=DEV))
    out = torch.full((D,), float("nan"), dtype=torch.float64, device=DEV)
    _udrlib.call("dvae_udr_kl_dims", m.data_ptr(), lv.data_ptr(), None if r is None else r.data_ptr(), N, D, S, ws.data_ptr(),
                 out.data_ptr(), stream())
    return out.cpu().numpy()


def assert_ranks(table, want, rows=None, what=""):
    got = run_ranks(table, rows)
    assert got.dtype == np.float32 and got.shape == want.shape
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d of %d ranks differ, first at %s: got %r, want %r" % (what, len(bad), got.size, bad[0], got[tuple(bad[0])],
                                                                                           want[tuple(bad[0])]))
    return got


# ---- 1. ranks, bit-exact ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,D", R.size_cases(_udrlib))
@pytest.mark.parametrize("kind", ["gauss", "quarters"])
def test_ranks_at_sizes(kind, S, D):
    table, want = R.rank_case(kind, S, D)
    assert_ranks(table, want, what="%s S %d D %d" % (kind, S, D))


@pytest.mark.parametrize("S,D", R.switch_cases(_udrlib))
@pytest.mark.parametrize("kind", ["gauss", "quarters"])
def test_ranks_on_both_sides_of_every_switch(kind, S, D):
    table, want = R.rank_case(kind, S, D)
    assert_ranks(table, want, what="%s S %d D %d" % (kind, S, D))


@pytest.mark.parametrize("S", [300, 2 * _udrlib.CHUNK_ROWS + 4], ids=["one workgroup", "three chunks"])
@pytest.mark.parametrize("kind", R.HARD)
def test_ranks_of_tables_built_to_break_a_radix_sort(kind, S):
    table, want = R.rank_case(kind, S, 3)
    got = assert_ranks(table, want, what="%s S %d" % (kind, S))
    if kind == "const":
        assert (got == (S + 1) / 2).all()                           # one run of length S, across every chunk
    if kind == "zeros":
        zero = table[:, 0] == 0
        assert len(np.unique(got[zero, 0])) == 1 and np.signbit(table[zero, 0]).any() and not np.signbit(table[zero, 0]).all()


@pytest.mark.parametrize("S", [500, 2 * _udrlib.CHUNK_ROWS + 4], ids=["one workgroup", "three chunks"])
def test_ranks_of_selected_rows(S):
    """rows with repeats tie with themselves; rows out of order give the ranks in the order of the selection"""
    table = R.hard_table("gauss", 700, 5)
    rng = np.random.default_rng(S)
    for rows in (rng.integers(0, 700, size=S), np.concatenate([np.arange(699, 300, -3), np.array([699, 0, 699, 0])])):
        want = R.ranks(table, rows).astype(np.float32)
        got = assert_ranks(table, want, rows)
        first = {}
        for s, row in enumerate(rows):
            assert got[s].tobytes() == got[first.setdefault(int(row), s)].tobytes()
        assert (got % 1 == 0.5).any()


def test_ranks_do_not_depend_on_what_the_workspace_held():
    for S in (700, _udrlib.SMALL_ROWS + 77):
        table, want = R.rank_case("quarters", S, 10)
        a, b, c = run_ranks(table, fill=NAN_A), run_ranks(table, fill=NAN_A), run_ranks(table, fill=NAN_B)
        assert a.tobytes() == b.tobytes() == c.tobytes() == want.tobytes()


# ---- 2. KL per dimension ------------------------------------------------------------------------------------------------------
def assert_kl(mean, logvar, rows=None):
    got, ref, tol = run_kl(mean, logvar, rows), R.kl_dims(mean, logvar, rows), R.kl_tolerance(mean, logvar, rows)
    ratio = np.abs(got - ref) / tol
    print("kl: worst err / tol %.4f" % ratio.max())
    assert got.dtype == np.float64 and np.isfinite(got).all() and ratio.max() <= 1.0, (got, ref, tol)
    assert run_kl(mean, logvar, rows).tobytes() == got.tobytes()
    return got


@pytest.mark.parametrize("kind", ["sharp", "edges"])
@pytest.mark.parametrize("B,D", [(1, 1), (63, 3), (300, 10), (3 * _udrlib.KL_BLOCK_ROWS - 5, 64), (21 * _udrlib.KL_BLOCK_ROWS + 1, 17)])
def test_kl_dims_vs_fp64(kind, B, D):
    if kind == "edges" and B < 4:
        B = 4
    _z, mu, logvar, _eps = LR.family(kind, B, D, seed=B + D)
    mu, logvar = mu.numpy(), logvar.numpy()
    if kind == "edges":
        assert logvar.max() == 4.0 and (D == 1 or logvar.min() == -20.0)      # D = 1: the one dimension ends at +4
    got = assert_kl(mu, logvar)
    if kind == "sharp":                                              # informative / collapsed, as the KL threshold tells them apart
        A = LR.n_active(D)
        assert (got[:A] > 1.0).all() and (got[A:] < 0.01).all()


@pytest.mark.parametrize("S", R.kl_switch_cases(_udrlib))
def test_kl_dims_on_both_sides_of_every_switch(S):
    _z, mu, logvar, _eps = LR.family("edges", 300, 3, seed=S)
    rows = np.random.default_rng(S).integers(0, 300, size=S)
    assert_kl(mu.numpy(), logvar.numpy(), rows)


# ---- 3. memory contract -------------------------------------------------------------------------------------------------------
def _udr_call(name):
    def fn(args):
        _udrlib.call(name, *[a.ptr if isinstance(a, Guarded) else a for a in args])
    return fn


# (N, D, S): the one-workgroup path, all rows and a selection; the chunked path (two chunks; three with a selection)
CONTRACT_SHAPES = [(60, 3, None), (700, 17, 65), (_udrlib.SMALL_ROWS + 1, 3, None), (700, 5, 2 * _udrlib.CHUNK_ROWS + 4)]


@pytest.mark.parametrize("N,D,S", CONTRACT_SHAPES)
def test_memory_contract_ranks(N, D, S):
    """Guards untouched, inputs unchanged, EVERY element of ranks written, bits equal to the run on plain tensors whatever the
    workspace and the surroundings hold; everything at 4-byte alignment, rows at 8."""
    table = R.hard_table("quarters", N, D)
    rows = None if S is None else np.random.default_rng(S).integers(0, N, size=S)
    n_sel = N if S is None else S
    nws = _udrlib.lib().dvae_udr_ranks_ws_floats(N, D, n_sel)

    def build(al):
        r = None if rows is None else al.inp("rows", rows.astype(np.int64), align=8)
        return [al.inp("table", table, align=4), r, N, D, n_sel, al.ws("ws", (nws,), align=4), al.out("ranks", (n_sel, D), align=4), stream()]
    runs = run_contract("dvae_udr_ranks", build, fn=_udr_call("dvae_udr_ranks"))
    assert runs[0].args[-1].t.cpu().numpy().tobytes() == R.ranks(table, rows).astype(np.float32).tobytes()


@pytest.mark.parametrize("N,D,S", [(60, 3, None), (700, 17, 65), (700, 5, 2 * _udrlib.KL_BLOCK_ROWS + 3)])
def test_memory_contract_kl_dims(N, D, S):
    _z, mu, logvar, _eps = LR.family("edges", N, D, seed=N)
    mu, logvar = mu.numpy(), logvar.numpy()
    rows = None if S is None else np.random.default_rng(S).integers(0, N, size=S)
    n_sel = N if S is None else S
    nws = _udrlib.lib().dvae_udr_kl_dims_ws_floats(N, D, n_sel)

    def build(al):
        r = None if rows is None else al.inp("rows", rows.astype(np.int64), align=8)
        return [al.inp("mean", mu, align=4), al.inp("logvar", logvar, align=4), r, N, D, n_sel, al.ws("ws", (nws,), align=4),
                al.out("kl", (D,), dtype=torch.float64, align=8), stream()]
    runs = run_contract("dvae_udr_kl_dims", build, fn=_udr_call("dvae_udr_kl_dims"))
    got = runs[0].args[-1].t.cpu().numpy()
    assert (np.abs(got - R.kl_dims(mu, logvar, rows)) <= R.kl_tolerance(mu, logvar, rows)).all()


# ---- 4. udr_from_tables -------------------------------------------------------------------------------------------------------
def _to_dev(tables):
    return [torch.from_numpy(t).to(DEV) for t in tables]


def assert_udr(got, means, logvars, correlation, rows=None, **kw):
    """got against the restatement at the tolerances of tests/udr_ref.py -> the restatement"""
    ref = R.udr(means, logvars, correlation, rows=rows, **kw)
    M, D = len(means), means[0].shape[1]
    assert set(got) == KEYS and got["correlation"] == correlation and got["n_samples"] == ref["n_samples"]
    assert isinstance(got["n_samples"], int) and got["raw_correlations"].shape == (M, M, D, D) and got["kl"].shape == (M, D)
    for i in range(M):
        assert (np.abs(got["kl"][i] - ref["kl"][i]) <= R.kl_tolerance(means[i], logvars[i], rows)).all()
    assert np.array_equal(got["n_active"], ref["n_active"])
    mask = ref["kl"] > kw.get("kl_threshold", 0.01)
    worst_R = worst_s = tol_max = 0.0
    for i in range(M):
        assert got["pairwise_scores"][i, i] == 0.0 and not got["raw_correlations"][i, i].any()
        for j in range(M):
            if i == j:
                continue
            if correlation == "spearman":
                tol = R.correlation_tolerance(R.ranks(means[i], rows), R.ranks(means[j], rows))
            else:
                tol = R.lasso_tolerance(means[i], means[j], mask[i], mask[j], kw.get("lasso_alpha", 0.1), rows)
            err = np.abs(got["raw_correlations"][i, j] - ref["raw_correlations"][i, j])
            dead = ~np.outer(mask[i], mask[j])
            assert not got["raw_correlations"][i, j][dead].any()                   # exact zeros where a latent is masked out
            assert (err <= tol).all(), (i, j, err.max(), tol.max())
            live = ~dead & (tol > 0)
            worst_R = max(worst_R, (err[live] / tol[live]).max() if live.any() else 0.0)
            tol_s = R.score_tolerance(tol, D)
            err_s = abs(got["pairwise_scores"][i, j] - ref["pairwise_scores"][i, j])
            assert err_s <= tol_s, (i, j, err_s, tol_s)
            worst_s, tol_max = max(worst_s, err_s / tol_s if tol_s else 0.0), max(tol_max, tol_s)
    assert (np.abs(got["model_scores"] - ref["model_scores"]) <= tol_max).all()
    print("%s: worst err / tol: R %.4f, pair scores %.4f (tol %.3g)" % (correlation, worst_R, worst_s, tol_max))
    return ref


@pytest.mark.parametrize("correlation", ["spearman", "lasso"])
@pytest.mark.parametrize("kind,D", R.END_TO_END)
def test_udr_from_tables_vs_fp64(kind, D, correlation):
    means, logvars = R.sweep(kind, D)
    got = udr_from_tables(_to_dev(means), _to_dev(logvars), correlation=correlation)
    ref = assert_udr(got, means, logvars, correlation)
    print(kind, D, correlation, got["model_scores"], ref["model_scores"])
    again = udr_from_tables(_to_dev(means), _to_dev(logvars), correlation=correlation)
    assert all(np.array_equal(np.asarray(got[k]), np.asarray(again[k])) for k in got)
    if kind == "rotated":                                            # the aligned sweep outranks its rotated copy, as in the restatement
        base = udr_from_tables(_to_dev(R.sweep("aligned", D)[0]), _to_dev(R.sweep("aligned", D)[1]), correlation=correlation)
        assert base["model_scores"][1] > got["model_scores"][1] + 0.2 and base["model_scores"].min() > 0.6


def test_udr_lasso_takes_the_gram_matrix_of_the_restatement():
    """the Pearson blocks of dvae_unsup_moments on the raw means ARE X^T X / S and X^T Y / S of the standardised representations,
    within the propagated bound of the moments"""
    means, logvars = R.sweep("aligned", 10)
    S, D = means[0].shape
    both = dev(torch.from_numpy(np.concatenate(means[:2], axis=1)))
    ws = keep(torch.empty(_unsuplib.lib().dvae_unsup_moments_ws_floats(S, 2 * D, S), device=DEV))
    lo, hi = torch.empty(2 * D, device=DEV), torch.empty(2 * D, device=DEV)
    mean, cov = torch.empty(2 * D, dtype=torch.float64, device=DEV), torch.empty(2 * D, 2 * D, dtype=torch.float64, device=DEV)
    _unsuplib.call("dvae_unsup_moments", both.data_ptr(), None, S, 2 * D, S, ws.data_ptr(), lo.data_ptr(), hi.data_ptr(), mean.data_ptr(),
                   cov.data_ptr(), stream())
    cov = cov.cpu().numpy()
    corr = cov / np.sqrt(np.outer(np.diag(cov), np.diag(cov)))
    x, y = (R.standardised(m, np.ones(D, bool)) for m in means[:2])
    raw = [m.astype(np.float64) for m in means[:2]]
    assert (np.abs(corr[:D, :D] - x.T @ x / S) <= R.gram_tolerance(raw[0])).all()
    assert (np.abs(corr[:D, D:] - x.T @ y / S) <= R.correlation_tolerance(raw[0], raw[1])).all()


def test_udr_model_without_an_informative_latent_scores_zero():
    means, logvars = R.sweep("collapsed", 3)
    for correlation in ("spearman", "lasso"):
        got = udr_from_tables(_to_dev(means), _to_dev(logvars), correlation=correlation)
        assert_udr(got, means, logvars, correlation)
        assert list(got["n_active"]) == [2, 2, 0] and got["model_scores"][2] == 0.0
        assert not got["pairwise_scores"][2].any() and not got["pairwise_scores"][:, 2].any() and got["pairwise_scores"][0, 1] > 0.5
        loose = udr_from_tables(_to_dev(means), _to_dev(logvars), correlation=correlation, filter_low_kl=False)
        assert_udr(loose, means, logvars, correlation, filter_low_kl=False)


def test_udr_seeds_rows_and_random_states():
    means, logvars = R.sweep("aligned", 10)
    dm, dl = _to_dev(means), _to_dev(logvars)
    cpu0, dev0 = torch.get_rng_state(), torch.cuda.get_rng_state()
    a, b, c = (udr_from_tables(dm, dl, n_samples=500, seed=s) for s in (3, 3, 4))
    assert torch.equal(torch.get_rng_state(), cpu0) and torch.equal(torch.cuda.get_rng_state(), dev0)
    assert a["n_samples"] == 500 and not np.array_equal(a["raw_correlations"], c["raw_correlations"])
    assert all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in a)
    gen = torch.Generator(device=DEV).manual_seed(3)                # the documented draw: randperm(N)[:n_samples], one for every model
    rows = torch.randperm(2000, generator=gen, device=DEV)[:500]
    d = udr_from_tables(dm, dl, rows=rows)
    assert all(np.array_equal(np.asarray(a[k]), np.asarray(d[k])) for k in a)
    assert_udr(a, means, logvars, "spearman", rows=rows.cpu().numpy())
    e = udr_from_tables(dm, dl, rows=rows, correlation="lasso")
    assert_udr(e, means, logvars, "lasso", rows=rows.cpu().numpy())


def test_udr_of_more_models_than_one_moments_call_holds():
    """M D > 64: a dvae_unsup_moments call per pair, the same scores as the one call gives where both apply"""
    means, logvars = R.sweep("aligned", 10, 2000, 7)
    got = udr_from_tables(_to_dev(means), _to_dev(logvars))
    assert_udr(got, means, logvars, "spearman")
    six = udr_from_tables(_to_dev(means[:6]), _to_dev(logvars[:6]))
    assert np.abs(six["pairwise_scores"] - got["pairwise_scores"][:6, :6]).max() <= 1e-12


# ---- 5. Evaluator end to end --------------------------------------------------------------------------------------------------
class _Images:
    """a data set WITHOUT known factors: no lat_sizes, no lat_names"""

    def __init__(self, images):
        self.images = images

    def __len__(self):
        return self.images.shape[0]


class _Loader:
    def __init__(self, images, bs, order=None):
        self.dataset, self.bs = _Images(images), bs
        self.order = torch.arange(len(self.dataset)) if order is None else order

    def __len__(self):
        return (len(self.dataset) + self.bs - 1) // self.bs

    def __iter__(self):
        for i in range(0, len(self.dataset), self.bs):
            yield self.dataset.images[self.order[i:i + self.bs]], 0


def test_evaluator_end_to_end(tmp_path):
    img, N, D = (1, 32, 32), 96, 4
    models = []
    for seed in (3, 4, 5):
        torch.manual_seed(seed)
        models.append(init_specific_model("Burgess", img, D))
    loss_f = get_loss_f("btcvae", device=torch.device(DEV), n_data=N, rec_dist="bernoulli", reg_anneal=0, btcvae_A=1, btcvae_B=6,
                        btcvae_G=1)
    images = torch.rand((N,) + img, generator=torch.Generator().manual_seed(4))
    order = torch.randperm(N, generator=torch.Generator().manual_seed(5))
    plain = _Loader(images, 32)
    assert not hasattr(plain.dataset, "lat_sizes")
    ev = Evaluator(models[0], loss_f, device=torch.device(DEV), logger=logging.getLogger("u"), save_dir=str(tmp_path),
                   is_progress_bar=False)
    models[0].train(), models[1].eval(), models[2].train()
    got = ev.compute_udr(plain, models[1:], kl_threshold=0.0)
    assert [m.training for m in models] == [True, False, True]      # the modes of all models are restored
    tables = []
    for m in models:
        m.eval()
        with torch.no_grad():
            tables.append(m.encoder(images.to(DEV)))
    models[0].train(), models[2].train()
    means, logvars = [t[0].cpu().numpy() for t in tables], [t[1].cpu().numpy() for t in tables]
    want = udr_from_tables([t[0] for t in tables], [t[1] for t in tables], kl_threshold=0.0)
    assert set(got) == KEYS and got["n_samples"] == N and got["model_scores"].shape == (3,)
    ref = assert_udr(got, means, logvars, "spearman", kl_threshold=0.0)
    assert_udr(want, means, logvars, "spearman", kl_threshold=0.0)
    # a shuffling loader: every batch goes through every model, so the rows of the tables line up whatever the order is.  The
    # native encoder treats the images of a batch in pairs and rounds the two of a pair differently (4e-7 of the means when an image
    # moves from an even to an odd place, nothing when it moves by an even number of places or to another batch), so after an
    # arbitrary shuffle the tables themselves differ: such a run is judged against the restatement on the tables encoded in ITS order
    mixed = ev.compute_udr(_Loader(images, 32, order), models[1:], kl_threshold=0.0)
    for m in models:
        m.eval()
    with torch.no_grad():
        enc = [[m.encoder(x.to(DEV)) for x, _ in _Loader(images, 32, order)] for m in models]
    models[0].train(), models[2].train()
    assert_udr(mixed, [torch.cat([mu for mu, _ in e]).cpu().numpy() for e in enc], [torch.cat([lv for _, lv in e]).cpu().numpy() for e in enc],
               "spearman", kl_threshold=0.0)
    # ... and a shuffle of the batches and, inside each, of the even and of the odd places among themselves changes only the row
    # order: the same scores within the bound
    g = torch.Generator().manual_seed(6)
    keeps = torch.cat([32 * b + torch.stack([2 * torch.randperm(16, generator=g), 2 * torch.randperm(16, generator=g) + 1], dim=1).reshape(-1)
                       for b in torch.randperm(3, generator=g).tolist()])
    assert sorted(keeps.tolist()) == list(range(N)) and (keeps % 2 == torch.arange(N) % 2).all() and not torch.equal(keeps, torch.arange(N))
    moved = ev.compute_udr(_Loader(images, 32, keeps), models[1:], kl_threshold=0.0)
    assert_udr(moved, [m[keeps.numpy()] for m in means], [lv[keeps.numpy()] for lv in logvars], "spearman", kl_threshold=0.0)
    tol = max(R.score_tolerance(R.correlation_tolerance(R.ranks(means[i]), R.ranks(means[j])), D) for i in range(3) for j in range(3) if i != j)
    assert np.abs(moved["pairwise_scores"] - got["pairwise_scores"]).max() <= 2 * tol
    assert np.abs(moved["model_scores"] - got["model_scores"]).max() <= 2 * tol
    part = ev.compute_udr(plain, models[1:], n_samples=40, seed=1, correlation="lasso")
    assert part["n_samples"] == 40 and part["correlation"] == "lasso"
    # Evaluator.__call__: with its defaults exactly the file it wrote before; udr.log only when udr_models is given
    _none, losses = ev(plain)
    assert sorted(os.listdir(tmp_path)) == ["test_losses.log"]
    metric, again = ev(plain, udr_models=models[1:])
    assert metric is None and set(again) == set(losses) and all(abs(again[k] - losses[k]) <= 1e-6 * abs(losses[k]) for k in losses)
    assert sorted(os.listdir(tmp_path)) == ["test_losses.log", "udr.log"]
    logged = json.load(open(tmp_path / "udr.log"))
    assert set(logged) == KEYS - {"raw_correlations"}
    full = ev.compute_udr(plain, models[1:])
    assert logged["n_samples"] == N and logged["correlation"] == "spearman" and logged["kl"] == full["kl"].tolist()
    assert logged["model_scores"] == full["model_scores"].tolist() and logged["n_active"] == full["n_active"].tolist()
    assert ev(plain, is_losses=False, udr_models=models[1:]) == (None, None)
    assert [m.training for m in models] == [True, False, True]
    assert _lib.lib().dvae_version() == 109
