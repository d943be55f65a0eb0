"""-m gpu: the FactorVAE / beta-VAE score kernels (libdvae_score_hip.so, csrc/factor_scores.hip) and
Evaluator.compute_factor_scores against the fp64 restatement of tests/scores_ref.py -- kernel parity on both sides of every
dispatch switch (row widths 4 / 16 / 64 and a second piece of 64, one wave / one workgroup per group, vote counters in LDS /
one thread per counter), the memory contract of the three launching entry points, and the scores end to end.

Tolerances.  Variance: |got - ref| <= 1e-5 ref + 4 * 2^-24 * max|x| * sqrt(ref) (max over the group's column): the project's
tolerance for reduced quantities plus the rounding of the fp32 group mean carried into the deviations; with inv_scale the same
times the scale.  Mean absolute pair difference: rtol 1e-5.  Votes and arg-mins: exact."""
import functools
import json
import logging
import math

import numpy as np
import pytest
import torch

import scores_ref as R
from gpu_util import DEV, dev, keep, stream
from guard_util import Guarded, run_contract
from disvae_amd import _lib, _scorelib, Evaluator
from disvae_amd.evaluate import factor_scores_from_table
from disvae_amd.models.losses import get_loss_f
from disvae_amd.models.vae import init_specific_model

pytestmark = pytest.mark.gpu
W = _scorelib.WAVE_MAX_L
BINS = _scorelib.VOTE_LDS_BINS

# (N, D, V, L).  D: 1, 3 -> width 4; 10, 16 -> 16; 17, 33 -> 64; 70 -> 64 and a second piece.  L <= W: a group per wave (V = 7 and
# V = 1 leave the last workgroup of four groups partly empty, V = 1000 fills 250); L > W: a group per workgroup.
SHAPES = [(4096, 10, 1000, 64), (4096, 10, 7, 63), (4096, 10, 7, 65), (300, 10, 7, 2), (4096, 10, 7, W), (4096, 10, 7, W + 1),
          (4096, 10, 1, 10000), (50, 1, 7, 64), (50, 1, 1, W + 1), (777, 3, 1000, 64), (4096, 3, 7, W + 1), (4096, 16, 7, 64),
          (4096, 16, 1, 1000), (4096, 17, 7, W), (4096, 17, 1, W + 1), (1000, 33, 7, 65), (1000, 33, 7, 300), (500, 70, 7, 64),
          (500, 70, 1, W + 1), (2000, 10, 1000, W + 1)]
OFFSET_SHAPES = [(4096, 10, 7, 64), (4096, 10, 1, 10000)]
CASES = [s + ("plain",) for s in SHAPES] + [s + ("offset",) for s in OFFSET_SHAPES]


@functools.lru_cache(maxsize=None)
def problem(N, D, V, L, family):
    """Table, rows and scale (fp32 / int64, CPU) with their fp64 statistics: computed once, shared, never modified."""
    rng = np.random.default_rng(1000 * D + L + V)
    table = (rng.standard_normal((N, D)) * rng.uniform(0.01, 2.0, size=D) + rng.uniform(-1, 1, size=D)).astype(np.float32)
    if family == "offset":
        table[:, D // 2] += np.float32(30.0)
    rows, rows_b = rng.integers(0, N, size=(V, L)), rng.integers(0, N, size=(V, L))
    scale = rng.uniform(0.5, 50.0, size=D).astype(np.float32)
    x = table.astype(np.float64)[rows]
    return {"table": table, "rows": rows, "rows_b": rows_b, "scale": scale, "var": R.group_var(table, rows),
            "absmax": np.abs(x).max(axis=1), "absdiff": R.pair_absdiff(table, rows, rows_b)}


def run_group_var(table, rows, scale=None):
    (N, D), (V, L) = table.shape, rows.shape
    assert 0 <= rows.min() and rows.max() < N                      # the kernels trust the rows
    t, r = dev(torch.from_numpy(table)), keep(torch.from_numpy(rows).to(DEV))
    s = None if scale is None else dev(torch.from_numpy(scale))
    need = _scorelib.lib().dvae_score_group_var_ws_floats(N, D, V, L)
    ws = keep(torch.full((max(need, 1),), float("nan"), device=DEV))
    out = torch.full((V, D), float("nan"), device=DEV)
    _scorelib.call("dvae_score_group_var", t.data_ptr(), r.data_ptr(), N, D, V, L, None if s is None else s.data_ptr(), ws.data_ptr(),
                   out.data_ptr(), stream())
    return out.cpu().double().numpy()


def run_pair_absdiff(table, rows_a, rows_b):
    (N, D), (V, L) = table.shape, rows_a.shape
    assert 0 <= min(rows_a.min(), rows_b.min()) and max(rows_a.max(), rows_b.max()) < N
    t, a, b = dev(torch.from_numpy(table)), keep(torch.from_numpy(rows_a).to(DEV)), keep(torch.from_numpy(rows_b).to(DEV))
    out = torch.full((V, D), float("nan"), device=DEV)
    _scorelib.call("dvae_score_pair_absdiff", t.data_ptr(), a.data_ptr(), b.data_ptr(), N, D, V, L, out.data_ptr(), stream())
    return out.cpu().double().numpy()


def var_tolerance(ref, absmax):
    return 1e-5 * ref + 4 * 2.0 ** -24 * absmax * np.sqrt(ref)


def assert_var(got, ref, absmax, what, scale=1.0):
    tol = var_tolerance(ref, absmax) * scale
    err = np.abs(got - ref * scale)
    print("%s: worst err / tol %.3f (max rel err %.2e)" % (what, (err / tol).max(), (err / (ref * scale)).max()))
    assert np.isfinite(got).all() and (err <= tol).all(), (what, (err / tol).max())


# ---- 1. kernel parity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,V,L,family", CASES)
def test_group_var_vs_fp64(N, D, V, L, family):
    p = problem(N, D, V, L, family)
    what = "group_var N%d D%d V%d L%d %s" % (N, D, V, L, family)
    assert_var(run_group_var(p["table"], p["rows"]), p["var"], p["absmax"], what)
    assert_var(run_group_var(p["table"], p["rows"], p["scale"]), p["var"], p["absmax"], what + " scaled",
               scale=p["scale"].astype(np.float64)[None, :])


@pytest.mark.parametrize("N,D,V,L,family", CASES)
def test_pair_absdiff_vs_fp64(N, D, V, L, family):
    p = problem(N, D, V, L, family)
    got = run_pair_absdiff(p["table"], p["rows"], p["rows_b"])
    rel = np.abs(got - p["absdiff"]) / p["absdiff"]
    print("pair_absdiff N%d D%d V%d L%d %s: worst rel err %.2e" % (N, D, V, L, family, rel.max()))
    np.testing.assert_allclose(got, p["absdiff"], rtol=1e-5)
    if L == 64:                                                    # a = b: exactly zero; L = 1: the difference itself
        assert (run_pair_absdiff(p["table"], p["rows"], p["rows"]) == 0).all()
        one = run_pair_absdiff(p["table"], p["rows"][:, :1].copy(), p["rows_b"][:, :1].copy())
        assert (one == np.abs(p["table"][p["rows"][:, 0]] - p["table"][p["rows_b"][:, 0]]).astype(np.float64)).all()


def test_group_var_of_a_constant_group_is_zero_and_rows_may_repeat():
    p = problem(4096, 10, 7, 64, "offset")
    rows = np.repeat(p["rows"][:, :1], 64, axis=1)                 # one row 64 times: deviations are exactly 0
    assert (run_group_var(p["table"], rows) == 0).all()


# ---- 2. the vote ---------------------------------------------------------------------------------------------------------------
def run_vote(stat, factor, active, K):
    V, D = stat.shape
    assert factor.min() >= 0 and factor.max() < K                  # the kernel trusts the factors
    s, f, a = dev(torch.from_numpy(stat)), keep(torch.from_numpy(factor).to(DEV)), keep(torch.from_numpy(active).to(DEV))
    argmin = torch.full((V,), -7, dtype=torch.int32, device=DEV)
    votes = torch.full((K, D), -7, dtype=torch.int32, device=DEV)
    _scorelib.call("dvae_score_vote", s.data_ptr(), f.data_ptr(), a.data_ptr(), V, D, K, argmin.data_ptr(), votes.data_ptr(), stream())
    return argmin.cpu().numpy(), votes.cpu().numpy()


# (V, D, K).  K * D <= BINS: counters in LDS (4 x 2048 is the last such size); above: one thread per counter.
VOTE_SHAPES = [(1, 1, 1), (1, 10, 5), (10007, 10, 5), (10007, 33, 1), (300, 33, 5), (300, 1, 5), (5, BINS // 4, 4),
               (5, BINS // 4 + 1, 4), (7, 2000, 5)]


@pytest.mark.parametrize("V,D,K", VOTE_SHAPES)
def test_vote_vs_numpy(V, D, K):
    rng = np.random.default_rng(V + D + K)
    stat = rng.integers(0, 4, size=(V, D)).astype(np.float32)      # few distinct values: exact ties everywhere
    active = (rng.random(D) < 0.7).astype(np.int32)
    active[0] = 1
    if D > 2:
        active[1] = 0
        stat[:, 1] = -5.0                                          # an inactive column holds the smallest value
        stat[::3, 0] = np.nan                                      # NaN in an active column
        stat[::5, 2] = np.inf
    factor = rng.integers(0, K, size=V).astype(np.int32)
    argmin, votes = run_vote(stat, factor, active, K)
    ref_argmin, ref_votes = R.vote(stat, factor, active, K)
    assert np.array_equal(argmin, ref_argmin) and np.array_equal(votes, ref_votes)
    assert votes.sum() == (ref_argmin >= 0).sum()
    if D > 2:
        assert not (argmin == 1).any()
    # no active column, and every active statistic NaN: all -1, all-zero votes
    for st, act in ((stat, np.zeros(D, dtype=np.int32)), (np.full((V, D), np.nan, dtype=np.float32), active)):
        argmin, votes = run_vote(st, factor, act, K)
        assert (argmin == -1).all() and (votes == 0).all()


# ---- 3. memory contract --------------------------------------------------------------------------------------------------------
def _score_call(name):
    def fn(args):
        _scorelib.call(name, *[a.ptr if isinstance(a, Guarded) else a for a in args])
    return fn


CONTRACT_SHAPES = [(300, 10, 7, 64), (300, 33, 3, W + 1), (50, 3, 5, W), (500, 70, 2, 300)]


@pytest.mark.parametrize("N,D,V,L", CONTRACT_SHAPES)
def test_memory_contract_group_var(N, D, V, L):
    """Guards untouched, inputs unchanged, every output element written, bits equal to the run on plain tensors whatever the
    workspace and the surroundings hold (NaN at 256-byte alignment; -1e30 at the weakest alignment promised: the element's own)."""
    p = problem(N, D, V, L, "plain")
    nws = max(_scorelib.lib().dvae_score_group_var_ws_floats(N, D, V, L), 1)

    def build(al):
        return [al.inp("table", p["table"], align=4), al.inp("rows", p["rows"], align=8), N, D, V, L,
                al.inp("inv_scale", p["scale"], align=4), al.ws("ws", (nws,), align=4), al.out("out", (V, D), align=4), stream()]
    run_contract("dvae_score_group_var", build, fn=_score_call("dvae_score_group_var"))


@pytest.mark.parametrize("N,D,V,L", CONTRACT_SHAPES)
def test_memory_contract_pair_absdiff(N, D, V, L):
    p = problem(N, D, V, L, "plain")

    def build(al):
        return [al.inp("table", p["table"], align=4), al.inp("rows_a", p["rows"], align=8), al.inp("rows_b", p["rows_b"], align=8),
                N, D, V, L, al.out("out", (V, D), align=4), stream()]
    run_contract("dvae_score_pair_absdiff", build, fn=_score_call("dvae_score_pair_absdiff"))


@pytest.mark.parametrize("V,D,K", [(300, 10, 5), (1, 1, 1), (7, 2000, 5)])
def test_memory_contract_vote(V, D, K):
    rng = np.random.default_rng(D)
    stat = rng.integers(0, 4, size=(V, D)).astype(np.float32)
    factor, active = rng.integers(0, K, size=V).astype(np.int32), (rng.random(D) < 0.7).astype(np.int32)

    def build(al):
        return [al.inp("stat", stat, align=4), al.inp("factor", factor, align=4), al.inp("active", active, align=4), V, D, K,
                al.out("argmin", (V,), dtype=torch.int32, align=4), al.out("votes", (K, D), dtype=torch.int32, align=4), stream()]
    run_contract("dvae_score_vote", build, fn=_score_call("dvae_score_vote"))


# ---- 4. the scores on tables whose answer is known -----------------------------------------------------------------------------
LAT = (3, 4, 5, 6)
N_TRAIN, N_EVAL, BATCH, DRAW_SEED = 2000, 1000, 64, 1


@functools.lru_cache(maxsize=None)
def reference(kind):
    draws = R.make_draws(LAT, N_TRAIN, N_EVAL, BATCH, 10000, seed=DRAW_SEED)
    return (draws,) + R.scores(R.synthetic_table(LAT, kind), LAT, draws)


def _torch_draws(draws):
    return {k: torch.from_numpy(v) if isinstance(v, np.ndarray) else tuple(torch.from_numpy(x) for x in v) for k, v in draws.items()}


def assert_votes(got, ref_det, draws, key, n):
    """The vote matrix equals the fp64 restatement's after leaving out the groups whose fp64 smallest and second-smallest
    normalised variances differ by less than 1e-4 relative: every other group votes as in fp64, each left-out group votes once,
    for its own factor.  More than 1 % left out fails.  Returns the number left out."""
    factor = draws["factor_vae_" + key][0]
    out = R.near_ties(ref_det["stat_" + key], ref_det["active"])
    assert out.sum() <= 0.01 * n, "%d of %d groups are near-ties" % (out.sum(), n)
    K = got.shape[0]
    kept = R.vote(ref_det["stat_" + key][~out], factor[~out], ref_det["active"], K)[1]
    extra = got - kept
    print("votes %s: %d groups left out" % (key, out.sum()))
    assert (extra >= 0).all() and np.array_equal(extra.sum(axis=1), np.bincount(factor[out], minlength=K)), (got, kept)
    return int(out.sum())


@pytest.mark.parametrize("kind", ["ideal", "rotated"])
def test_scores_from_table_vs_fp64(kind):
    """Rotated table: draws of seed 1 (scores_ref.make_draws), for which the fp64 restatement itself leaves out 0 of the 2000
    train and 0 of the 1000 eval groups (0.0 %; smallest relative gap 1.3e-4 / 4.8e-4, measured on the CPU).  Ideal table: the
    smallest gap is 0.998, nothing is left out."""
    draws, ref, ref_det = reference(kind)
    table = torch.from_numpy(R.synthetic_table(LAT, kind).copy()).to(DEV)
    got, det = factor_scores_from_table(table, LAT, n_train=N_TRAIN, n_eval=N_EVAL, batch_size=BATCH, draws=_torch_draws(draws),
                                        return_details=True)
    print(kind, got, ref)
    x = R.synthetic_table(LAT, kind).astype(np.float64)[draws["variance_rows"]]
    assert_var(det["var"].astype(np.float64), ref_det["var"], np.abs(x).max(axis=0), kind + " global variance")
    assert np.array_equal(det["active"], ref_det["active"]) and got["n_active"] == ref["n_active"] == len(LAT)
    left = {key: assert_votes(det["votes_" + key], ref_det, draws, key, n) for key, n in (("train", N_TRAIN), ("eval", N_EVAL))}
    np.testing.assert_allclose(det["features_train"].numpy(), ref_det["features_train"], rtol=1e-5)
    assert (got["n_train"], got["n_eval"], got["batch_size"]) == (N_TRAIN, N_EVAL, BATCH)
    if kind == "ideal":
        assert left == {"train": 0, "eval": 0}
        assert np.array_equal(det["votes_train"], ref_det["votes_train"]) and np.array_equal(det["votes_eval"], ref_det["votes_eval"])
        for k in ("factor_vae_train", "factor_vae_eval", "beta_vae_train", "beta_vae_eval"):
            assert got[k] == 1.0, (k, got[k])
    else:
        assert abs(got["factor_vae_train"] - ref["factor_vae_train"]) <= left["train"] / N_TRAIN + 1e-12
        assert abs(got["factor_vae_eval"] - ref["factor_vae_eval"]) <= left["eval"] / N_EVAL + 1e-12
        assert abs(got["beta_vae_train"] - ref["beta_vae_train"]) <= 2.0 / N_TRAIN + 1e-12
        assert abs(got["beta_vae_eval"] - ref["beta_vae_eval"]) <= 2.0 / N_EVAL + 1e-12
        assert got["factor_vae_train"] < 1.0 and got["factor_vae_eval"] < 1.0


def test_scores_from_table_seeds_and_random_states():
    table = torch.from_numpy(R.synthetic_table(LAT, "rotated").copy()).to(DEV)
    cpu0, dev0 = torch.get_rng_state(), torch.cuda.get_rng_state()
    kw = dict(n_train=300, n_eval=200, batch_size=32, n_variance=200)
    a, b, c = (factor_scores_from_table(table, LAT, seed=s, **kw) for s in (3, 3, 4))
    assert a == b and a != c
    assert torch.equal(torch.get_rng_state(), cpu0) and torch.equal(torch.cuda.get_rng_state(), dev0)
    assert all(0.0 <= a[k] <= 1.0 for k in ("factor_vae_train", "factor_vae_eval", "beta_vae_train", "beta_vae_eval"))
    with pytest.raises(ValueError, match=r"lie in \[0, 360\)"):
        factor_scores_from_table(table, LAT, draws={"variance_rows": torch.tensor([0, 360])}, **kw)
    with pytest.raises(ValueError, match="unknown draws"):
        factor_scores_from_table(table, LAT, draws={"variance": torch.tensor([0, 1])}, **kw)


# ---- 5. Evaluator end to end ---------------------------------------------------------------------------------------------------
class _FactorData:
    """tiny data set with known factors, iterated in factor order (what compute_factor_scores requires)."""
    lat_sizes = np.array([3, 4, 5])
    lat_names = ("a", "b", "c")

    def __init__(self, images):
        self.images = images

    def __len__(self):
        return self.images.shape[0]


class _Loader:
    def __init__(self, images, bs):
        self.dataset, self.bs = _FactorData(images), bs

    def __len__(self):
        return (len(self.dataset) + self.bs - 1) // self.bs

    def __iter__(self):
        for i in range(0, len(self.dataset), self.bs):
            yield self.dataset.images[i:i + self.bs], 0


def test_evaluator_end_to_end(tmp_path):
    img, N, lat = (1, 64, 64), 60, (3, 4, 5)
    kw = dict(n_train=200, n_eval=100, batch_size=16, n_variance=60)
    torch.manual_seed(3)
    model = init_specific_model("Burgess", img, 10)
    loss_f = get_loss_f("btcvae", device=torch.device(DEV), n_data=N, rec_dist="bernoulli", reg_anneal=0, btcvae_A=1, btcvae_B=6,
                        btcvae_G=1)
    # low-contrast images: the posterior means of a fresh (Kaiming-initialised) encoder then spread by ~0.008 per dimension,
    # far below the default threshold of 0.05 (uniform-noise images of full contrast spread them by ~0.29: all ten active)
    images = 0.5 + 0.02 * (torch.rand((N,) + img, generator=torch.Generator().manual_seed(4)) - 0.5)
    loader = _Loader(images, 16)
    ev = Evaluator(model, loss_f, device=torch.device(DEV), logger=logging.getLogger("s"), save_dir=str(tmp_path),
                   is_progress_bar=False)
    model.train()
    keys = ("factor_vae_train", "factor_vae_eval", "beta_vae_train", "beta_vae_eval")
    # a fresh model's posterior means barely move on these images: no dimension reaches the default threshold
    plain = ev.compute_factor_scores(loader, **kw)
    print("default threshold:", plain)
    assert model.training
    assert set(plain) == set(keys) | {"n_active", "n_train", "n_eval", "batch_size"}
    assert plain["n_active"] == 0 and plain["factor_vae_train"] == 0.0 and plain["factor_vae_eval"] == 0.0
    assert all(math.isfinite(plain[k]) and 0.0 <= plain[k] <= 1.0 for k in keys)
    assert (plain["n_train"], plain["n_eval"], plain["batch_size"]) == (200, 100, 16)
    assert plain == ev.compute_factor_scores(loader, **kw)                       # the same seed: the same dict
    # every dimension active, injected draws: the votes against fp64 on the table read back from the encoder
    draws = R.make_draws(lat, 200, 100, 16, 60, seed=2)
    got = ev.compute_factor_scores(loader, active_threshold=0.0, draws=_torch_draws(draws), **kw)
    model.eval()
    with torch.no_grad():
        mean, _ = model.encoder(images.to(DEV))
    model.train()
    again, det = factor_scores_from_table(mean, lat, active_threshold=0.0, draws=_torch_draws(draws), return_details=True, **kw)
    assert got == again and got["n_active"] == 10
    ref, ref_det = R.scores(mean.cpu().numpy(), lat, draws, active_threshold=0.0)
    print("threshold 0:", got, ref, "spread of the means", mean.std(0).tolist())
    assert ref_det["active"].all() and np.array_equal(det["active"], ref_det["active"])
    left = {}
    for key, n in (("train", 200), ("eval", 100)):
        factor = draws["factor_vae_" + key][0]
        out = R.near_ties(ref_det["stat_" + key], ref_det["active"])
        assert out.sum() <= 0.01 * n
        kept = R.vote(ref_det["stat_" + key][~out], factor[~out], ref_det["active"], 3)[1]
        extra = det["votes_" + key] - kept
        assert (extra >= 0).all() and np.array_equal(extra.sum(axis=1), np.bincount(factor[out], minlength=3))
        left[key] = int(out.sum())
    assert abs(got["factor_vae_train"] - ref["factor_vae_train"]) <= left["train"] / 200 + 1e-12
    assert abs(got["factor_vae_eval"] - ref["factor_vae_eval"]) <= left["eval"] / 100 + 1e-12
    # Evaluator.__call__: the file only on request, the return value the reference's
    ev(loader, is_losses=False)
    assert not (tmp_path / "factor_scores.log").exists()
    assert ev(loader, is_losses=False, is_scores=True) == (None, None)
    logged = json.load(open(tmp_path / "factor_scores.log"))
    assert set(logged) == set(plain) and logged["n_train"] == 10000 and logged["batch_size"] == 64 and logged["n_active"] == 0
    assert model.training

    class _NoFactors:
        dataset = [0, 1, 2, 3]
    with pytest.raises(ValueError, match="known true factors"):
        ev.compute_factor_scores(_NoFactors())
    assert _lib.lib().dvae_version() == 109
