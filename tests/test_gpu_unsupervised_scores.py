"""-m gpu: the covariance / pair-histogram kernels (libdvae_unsup_hip.so, csrc/latent_pairs.hip), unsupervised_scores_from_table
and Evaluator.compute_unsupervised_scores against the fp64 restatement of tests/unsup_ref.py -- every count exactly and the same
on a second run, min / max bit for bit, the covariance bitwise symmetric, mean and covariance inside the accumulation bound of
unsup_ref (8 S u sqrt(m2_d m2_e)), on both sides of every dispatch macro of include/dvae_unsup_hip.h (one workgroup / two, the
grid cap, one tile of pairs / two, one pair per tile, one sum per thread / two), the wave-uniform add, the memory contract of
the two launching entry points, and the scores end to end.

Measured on the MI355X, worst error / tolerance over all cases below: covariance 0.016, mean 0.018, the Gaussian scores end to end
0.24; the 52 tests take 5 s."""
import json
import logging
import os

import numpy as np
import pytest
import torch

import info_ref as I
import unsup_ref as R
from gpu_util import DEV, dev, keep, stream
from guard_util import Guarded, run_contract
from disvae_amd import _lib, _unsuplib, Evaluator
from disvae_amd.evaluate import unsupervised_scores_from_statistics, unsupervised_scores_from_table
from disvae_amd.models.losses import get_loss_f
from disvae_amd.models.vae import init_specific_model

pytestmark = pytest.mark.gpu

GAUSSIAN_KEYS = ("gaussian_total_correlation", "gaussian_wasserstein_correlation", "gaussian_wasserstein_correlation_norm")
KEYS = set(GAUSSIAN_KEYS) | {"mutual_info_score", "mutual_information", "active_units", "variances", "live", "n_samples", "n_bins"}


def _device_args(table, rows):
    N, D = table.shape
    if rows is not None:
        assert 0 <= rows.min() and rows.max() < N                  # the kernels trust the rows
    t = dev(torch.from_numpy(table))
    r = None if rows is None else keep(torch.from_numpy(rows.astype(np.int64)).to(DEV))
    return t, r, N, D, (N if rows is None else len(rows))


def run_moments(table, rows=None):
    t, r, N, D, S = _device_args(table, rows)
    need = _unsuplib.lib().dvae_unsup_moments_ws_floats(N, D, S)
    assert need > 0
    ws = keep(torch.full((need,), float("nan"), device=DEV))
    out = {"min": torch.full((D,), float("nan"), device=DEV), "max": torch.full((D,), float("nan"), device=DEV),
           "mean": torch.full((D,), float("nan"), dtype=torch.float64, device=DEV),
           "cov": torch.full((D, D), float("nan"), dtype=torch.float64, device=DEV)}
    _unsuplib.call("dvae_unsup_moments", t.data_ptr(), None if r is None else r.data_ptr(), N, D, S, ws.data_ptr(),
                   out["min"].data_ptr(), out["max"].data_ptr(), out["mean"].data_ptr(), out["cov"].data_ptr(), stream())
    return {k: v.cpu().numpy() for k, v in out.items()}


def run_hist(table, edges, rows=None):
    t, r, N, D, S = _device_args(table, rows)
    n_bins = edges.shape[1]
    e = dev(torch.from_numpy(edges))
    assert _unsuplib.lib().dvae_unsup_pair_hist_ws_floats(N, D, S, n_bins) == 0
    counts = torch.full((D * (D - 1) // 2, n_bins, n_bins), -7, dtype=torch.int32, device=DEV)
    _unsuplib.call("dvae_unsup_pair_hist", t.data_ptr(), None if r is None else r.data_ptr(), e.data_ptr(), N, D, S, n_bins, None,
                   counts.data_ptr(), stream())
    return counts.cpu().numpy()


def assert_case(lat_sizes, D, n_bins, family, S):
    c = R.case(lat_sizes, D, n_bins, family, S)
    what = "rows of %s D %d bins %d %s S %s" % (lat_sizes, D, n_bins, family, S)
    # ---- histograms: every count (one latent has no pair)
    if D > 1:
        got = run_hist(c["table"], c["edges"], c["rows"])
        assert got.dtype == np.int32 and np.array_equal(got, c["counts"]), what
        assert np.array_equal(run_hist(c["table"], c["edges"], c["rows"]), got), what + ": second run"
    # ---- moments
    ref, got = c["moments"], run_moments(c["table"], c["rows"])
    assert got["min"].tobytes() == ref["min"].tobytes() and got["max"].tobytes() == ref["max"].tobytes(), what
    assert got["cov"].dtype == np.float64 and got["mean"].dtype == np.float64
    assert got["cov"].tobytes() == np.ascontiguousarray(got["cov"].T).tobytes(), what + ": cov is not bitwise symmetric"
    ratio = {"cov": R.worst_ratio(got["cov"], ref["cov"], R.cov_tolerance(ref)),
             "mean": R.worst_ratio(got["mean"], ref["mean"], R.mean_tolerance(ref))}
    print("%s: err / tol %s" % (what, {k: round(v, 4) for k, v in ratio.items()}))
    assert ratio["cov"] <= 1.0 and ratio["mean"] <= 1.0, (what, ratio)
    again = run_moments(c["table"], c["rows"])
    assert all(again[k].tobytes() == got[k].tobytes() for k in got), what + ": second run"
    if ref["S"] == 1:
        assert not got["cov"].any() and got["mean"].tobytes() == c["table"][c["rows"][0]].astype(np.float64).tobytes()
    return ratio


# ---- 1. kernel parity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lat_sizes,D,n_bins,family,S", R.CASES)
def test_counts_and_moments_vs_fp64(lat_sizes, D, n_bins, family, S):
    assert_case(lat_sizes, D, n_bins, family, S)


@pytest.mark.parametrize("lat_sizes,D,n_bins,family,S", R.switch_cases(_unsuplib))
def test_counts_and_moments_on_both_sides_of_every_switch(lat_sizes, D, n_bins, family, S):
    assert_case(lat_sizes, D, n_bins, family, S)


def test_one_pair_hist_is_refused_for_one_latent():
    table = R.make_table((60,), 1, "gauss")
    with pytest.raises(_lib.DvaeHipError, match="invalid argument"):
        run_hist(table, R.pair_counts(table, 20)[1])


def test_waves_whose_rows_share_a_cell():
    """Two chunks of 2067 rows (8 blocks of 256 and 19 rows: the last wave of each chunk is partial).  64 consecutive rows in one cell
    at the start of each chunk, the 19 rows of the first chunk's partial wave in one cell too, gauss rows between them; column 1 is
    collapsed throughout, so (1, 3) is a pair of which whole waves share the cell only inside the runs."""
    S = _unsuplib.HIST_BLOCK_ROWS + 37
    chunk = (S + 1) // 2
    assert chunk % 256 == 19 and chunk % 64 == 19
    rng = np.random.default_rng(11)
    table = rng.standard_normal((S, 4)).astype(np.float32)
    table[:, 1] = np.float32(0.3)
    for start, n in ((0, 64), (chunk, 64), (chunk - 19, 19)):
        table[start:start + n] = table[start]
    counts, edges = R.pair_counts(table, 20)
    got = run_hist(table, edges)
    assert np.array_equal(got, counts) and got.sum() == 6 * S
    assert counts.max(axis=(1, 2)).min() >= 64                       # every pair has a cell that a run filled
    assert np.array_equal(run_hist(table, edges), got)


def test_selected_rows_out_of_order_give_the_counts_of_those_rows():
    table = R.make_table((2, 3, 6, 40), 5, "disent")
    rows = np.concatenate([np.arange(700, 300, -3), np.arange(5, 90, 7), np.array([1439, 0, 1439])])
    counts, edges = R.pair_counts(table, 20, rows)
    assert np.array_equal(run_hist(table, edges, rows), counts)
    full, _ = R.pair_counts(table, 20)
    assert not np.array_equal(run_hist(table, edges, rows), full)
    got, ref = run_moments(table, rows), R.moments(table, rows)
    assert got["min"].tobytes() == ref["min"].tobytes() and R.worst_ratio(got["cov"], ref["cov"], R.cov_tolerance(ref)) <= 1.0


# ---- 2. memory contract --------------------------------------------------------------------------------------------------------
def _unsup_call(name):
    def fn(args):
        _unsuplib.call(name, *[a.ptr if isinstance(a, Guarded) else a for a in args])
    return fn


# small; odd (17 columns, 7 bins, 65 selected rows); the first D whose pairs need two tiles at 20 bins
CONTRACT_SHAPES = [((3, 4, 5), 3, 20, None), ((2, 3, 6, 40), 17, 7, 65), ((3, 4, 5), R.tile_dims(_unsuplib)[1], 20, None)]


@pytest.mark.parametrize("lat_sizes,D,n_bins,S", CONTRACT_SHAPES)
def test_memory_contract_moments(lat_sizes, D, n_bins, S):
    """Guards untouched, inputs unchanged, every output element written, bits equal to the run on plain tensors whatever the
    workspace and the surroundings hold; the fp64 outputs at 8-byte alignment, everything else at its element's own."""
    c = R.case(lat_sizes, D, n_bins, "gauss", S)
    N = c["table"].shape[0]
    n_sel = N if S is None else S
    nws = _unsuplib.lib().dvae_unsup_moments_ws_floats(N, D, n_sel)

    def build(al):
        rows = None if S is None else al.inp("rows", c["rows"].astype(np.int64), align=8)
        return [al.inp("table", c["table"], align=4), rows, N, D, n_sel, al.ws("ws", (nws,), align=4), al.out("col_min", (D,), align=4),
                al.out("col_max", (D,), align=4), al.out("col_mean", (D,), dtype=torch.float64, align=8),
                al.out("cov", (D, D), dtype=torch.float64, align=8), stream()]
    runs = run_contract("dvae_unsup_moments", build, fn=_unsup_call("dvae_unsup_moments"))
    cov = runs[0].args[-1].t.cpu().numpy().reshape(D, D)
    assert R.worst_ratio(cov, c["moments"]["cov"], R.cov_tolerance(c["moments"])) <= 1.0


@pytest.mark.parametrize("lat_sizes,D,n_bins,S", CONTRACT_SHAPES)
def test_memory_contract_pair_hist(lat_sizes, D, n_bins, S):
    c = R.case(lat_sizes, D, n_bins, "gauss", S)
    N = c["table"].shape[0]
    n_sel = N if S is None else S

    def build(al):
        rows = None if S is None else al.inp("rows", c["rows"].astype(np.int64), align=8)
        return [al.inp("table", c["table"], align=4), rows, al.inp("edges", c["edges"], align=4), N, D, n_sel, n_bins,
                al.ws("ws", (1,), align=4), al.out("counts", (D * (D - 1) // 2, n_bins, n_bins), dtype=torch.int32, align=4), stream()]
    runs = run_contract("dvae_unsup_pair_hist", build, fn=_unsup_call("dvae_unsup_pair_hist"))
    assert np.array_equal(runs[0].args[-1].t.cpu().numpy().reshape(c["counts"].shape), c["counts"])


# ---- 3. the scores from a table ------------------------------------------------------------------------------------------------
def assert_scores(got, ref, mom):
    assert set(got) == KEYS and (got["n_samples"], got["n_bins"]) == (ref["n_samples"], ref["n_bins"])
    assert np.abs(got["mutual_information"] - ref["mutual_information"]).max() <= 1e-12       # exact counts, fp64 on the host
    assert abs(got["mutual_info_score"] - ref["mutual_info_score"]) <= 1e-12
    assert np.array_equal(got["live"], ref["live"]) and got["active_units"] == ref["active_units"]
    tol = R.score_tolerance(mom)
    worst = 0.0
    for key in GAUSSIAN_KEYS:
        if np.isinf(ref[key]):
            assert got[key] == ref[key], key
            continue
        err = abs(got[key] - ref[key])
        worst = max(worst, 0.0 if err == 0 else err / max(tol, 1e-300))
        assert err <= tol, (key, got[key], ref[key], tol)
    print("gaussian scores: worst err / tol %.4f (tol %.3g)" % (worst, tol))
    assert R.worst_ratio(got["variances"], ref["variances"], np.diag(R.cov_tolerance(mom))) <= 1.0
    assert isinstance(got["gaussian_total_correlation"], float) and isinstance(got["mutual_information"], np.ndarray)
    assert isinstance(got["n_samples"], int) and isinstance(got["active_units"], int)


@pytest.mark.parametrize("kind,lat_sizes,D,n_bins,S", R.END_TO_END)
def test_scores_from_table_vs_fp64(kind, lat_sizes, D, n_bins, S):
    table, rows = R.end_to_end_case(kind, lat_sizes, D, n_bins, S)
    got = unsupervised_scores_from_table(torch.from_numpy(table).to(DEV), n_bins=n_bins, rows=rows)
    print(kind, {k: v for k, v in got.items() if not isinstance(v, np.ndarray)})
    assert_scores(got, R.scores(table, n_bins, rows), R.moments(table, rows))
    # ... and it is the host combination applied to the kernels' own outputs, exactly
    mom = run_moments(table, rows)
    counts = run_hist(table, np.stack([I.lower_edges(R.select(table, rows)[:, d], n_bins) for d in range(D)]), rows) if D > 1 else None
    mine = unsupervised_scores_from_statistics(mom["min"], mom["max"], mom["cov"], counts, n_bins)
    for key in mine:
        assert np.array_equal(np.asarray(mine[key]), np.asarray(got[key])), key
    if kind == "const" or S == 1:
        assert all(got[k] == 0.0 for k in GAUSSIAN_KEYS) and got["mutual_info_score"] == 0.0 and not got["live"].any()
    if kind == "mixed" and S != 1:
        assert list(got["live"][:4]) == [True, False, True, True] and got["active_units"] < got["live"].sum()


def test_scores_from_table_seeds_and_random_states():
    table = torch.from_numpy(R.make_table((2, 3, 6, 40), 10, "gauss")).to(DEV)
    cpu0, dev0 = torch.get_rng_state(), torch.cuda.get_rng_state()
    a, b, c = (unsupervised_scores_from_table(table, n_samples=500, seed=s) for s in (3, 3, 4))
    assert torch.equal(torch.get_rng_state(), cpu0) and torch.equal(torch.cuda.get_rng_state(), dev0)
    assert a["n_samples"] == 500 and a["gaussian_total_correlation"] != c["gaussian_total_correlation"]
    assert not np.array_equal(a["mutual_information"], c["mutual_information"])
    assert all(np.array_equal(a[k], b[k]) for k in a)
    gen = torch.Generator(device=DEV).manual_seed(3)                # the documented draw: randperm(N)[:n_samples]
    rows = torch.randperm(1440, generator=gen, device=DEV)[:500]
    d = unsupervised_scores_from_table(table, rows=rows)
    assert all(np.array_equal(a[k], d[k]) for k in a)
    assert_scores(a, R.scores(table.cpu().numpy(), 20, rows.cpu().numpy()), R.moments(table.cpu().numpy(), rows.cpu().numpy()))
    bad = table.clone()
    bad[7, 2] = float("inf")
    with pytest.raises(ValueError, match="NaN or an infinity"):
        unsupervised_scores_from_table(bad)


# ---- 4. Evaluator end to end ---------------------------------------------------------------------------------------------------
class _Images:
    """a data set WITHOUT known factors: no lat_sizes, no lat_names"""

    def __init__(self, images):
        self.images = images

    def __len__(self):
        return self.images.shape[0]


class _Loader:
    def __init__(self, images, bs):
        self.dataset, self.bs = _Images(images), bs

    def __len__(self):
        return (len(self.dataset) + self.bs - 1) // self.bs

    def __iter__(self):
        for i in range(0, len(self.dataset), self.bs):
            yield self.dataset.images[i:i + self.bs], 0


def test_evaluator_end_to_end(tmp_path):
    img, N = (1, 32, 32), 96
    torch.manual_seed(3)
    model = init_specific_model("Burgess", img, 4)
    loss_f = get_loss_f("btcvae", device=torch.device(DEV), n_data=N, rec_dist="bernoulli", reg_anneal=0, btcvae_A=1, btcvae_B=6,
                        btcvae_G=1)
    images = torch.rand((N,) + img, generator=torch.Generator().manual_seed(4))
    loader = _Loader(images, 40)                                    # batches of 40 / 40 / 16
    assert [x.shape[0] for x, _ in loader] == [40, 40, 16] and not hasattr(loader.dataset, "lat_sizes")
    ev = Evaluator(model, loss_f, device=torch.device(DEV), logger=logging.getLogger("u"), save_dir=str(tmp_path),
                   is_progress_bar=False)
    model.train()
    got = ev.compute_unsupervised_scores(loader, n_bins=8)
    assert model.training
    model.eval()
    with torch.no_grad():
        mean, _ = model.encoder(images.to(DEV))
    model.train()
    want = unsupervised_scores_from_table(mean, n_bins=8)
    assert set(got) == KEYS and all(np.array_equal(np.asarray(got[k]), np.asarray(want[k])) for k in got)
    assert got["n_samples"] == N and got["mutual_information"].shape == (4, 4) and got["variances"].shape == (4,)
    table = mean.cpu().numpy()
    assert_scores(got, R.scores(table, 8), R.moments(table))
    part = ev.compute_unsupervised_scores(loader, n_samples=40, seed=1)
    assert part["n_samples"] == 40 and part["n_bins"] == 20
    # Evaluator.__call__: with its defaults exactly the file it wrote before; the new one only on request, without the matrix
    _none, losses = ev(loader)
    assert sorted(os.listdir(tmp_path)) == ["test_losses.log"]
    metric, again = ev(loader, is_unsupervised=True)                # the reference's (metric, losses), as without the flag
    assert metric is None and set(again) == set(losses) and all(abs(again[k] - losses[k]) <= 1e-6 * abs(losses[k]) for k in losses)
    assert sorted(os.listdir(tmp_path)) == ["test_losses.log", "unsupervised_scores.log"]
    logged = json.load(open(tmp_path / "unsupervised_scores.log"))
    assert set(logged) == KEYS - {"mutual_information"}
    full = ev.compute_unsupervised_scores(loader)
    assert logged["n_samples"] == N and logged["n_bins"] == 20 and logged["variances"] == full["variances"].tolist()
    assert logged["live"] == full["live"].tolist() and logged["gaussian_total_correlation"] == full["gaussian_total_correlation"]
    assert ev(loader, is_losses=False, is_unsupervised=True) == (None, None)
    assert model.training
    assert _lib.lib().dvae_version() == 109
