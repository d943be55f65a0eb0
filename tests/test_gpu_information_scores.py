"""-m gpu: the moments / joint-histogram kernels (libdvae_info_hip.so, csrc/factor_info.hip), information_scores_from_table and
Evaluator.compute_information_scores against the fp64 restatement of tests/info_ref.py -- every count exactly, min / max bit for
bit, means / variances / covariances inside the rule of info_ref (tolerance x max(1, 4 e32)), on both sides of every dispatch
macro of include/dvae_info_hip.h (lanes per row 4 / 16 / 64 and a second piece of 64, one workgroup / two, the grid cap,
counters in LDS / in global memory), the memory contract of the two launching entry points, and the scores end to end.

Measured on the MI355X, worst over all cases below: see DESIGN.md section 2."""
import json
import logging
import os

import numpy as np
import pytest
import torch

import info_ref as R
from gpu_util import DEV, dev, keep, stream
from guard_util import Guarded, run_contract
from disvae_amd import _infolib, _lib, Evaluator
from disvae_amd.evaluate import information_scores_from_table
from disvae_amd.models.losses import get_loss_f
from disvae_amd.models.vae import init_specific_model

pytestmark = pytest.mark.gpu

MOMENT_KEYS = ("min", "max", "mean", "var", "cov", "factor_mean", "factor_var")


def _device_args(table, lat_sizes, rows):
    N, D = table.shape
    if rows is not None:
        assert 0 <= rows.min() and rows.max() < N                  # the kernels trust the rows
    t = dev(torch.from_numpy(table))
    r = None if rows is None else keep(torch.from_numpy(rows.astype(np.int64)).to(DEV))
    sizes = keep(torch.tensor(lat_sizes, dtype=torch.int32, device=DEV))
    return t, r, sizes, N, D, len(lat_sizes), (N if rows is None else len(rows))


def run_moments(table, lat_sizes, rows=None):
    t, r, sizes, N, D, K, S = _device_args(table, lat_sizes, rows)
    need = _infolib.lib().dvae_info_moments_ws_floats(N, D, K, S)
    assert need > 0
    ws = keep(torch.full((need,), float("nan"), device=DEV))
    shapes = dict(min=(D,), max=(D,), mean=(D,), var=(D,), cov=(D, K), factor_mean=(K,), factor_var=(K,))
    out = {k: torch.full(shapes[k], float("nan"), device=DEV) for k in MOMENT_KEYS}
    _infolib.call("dvae_info_moments", t.data_ptr(), None if r is None else r.data_ptr(), sizes.data_ptr(), N, D, K, S, ws.data_ptr(),
                  *[out[k].data_ptr() for k in MOMENT_KEYS], stream())
    return {k: v.cpu().numpy() for k, v in out.items()}


def run_hist(table, lat_sizes, edges, rows=None):
    t, r, sizes, N, D, K, S = _device_args(table, lat_sizes, rows)
    n_bins, total = edges.shape[1], sum(lat_sizes)
    e = dev(torch.from_numpy(edges))
    need = _infolib.lib().dvae_info_hist_ws_floats(N, D, K, S, n_bins, total)
    ws = keep(torch.full((max(need, 1),), float("nan"), device=DEV))
    counts = torch.full((D, n_bins * total), -7, dtype=torch.int32, device=DEV)
    _infolib.call("dvae_info_joint_hist", t.data_ptr(), None if r is None else r.data_ptr(), sizes.data_ptr(), e.data_ptr(), N, D, K, S,
                  n_bins, total, ws.data_ptr(), counts.data_ptr(), stream())
    return counts.cpu().numpy()


def assert_case(lat_sizes, D, n_bins, family, S):
    c = R.case(lat_sizes, D, n_bins, family, S)
    what = "lat %s D %d bins %d %s S %s" % (lat_sizes, D, n_bins, family, S)
    # ---- histograms: every count
    got = run_hist(c["table"], lat_sizes, c["edges"], c["rows"])
    assert got.dtype == np.int32 and np.array_equal(got, c["counts"]), what
    assert np.array_equal(run_hist(c["table"], lat_sizes, c["edges"], c["rows"]), got), what + ": second run"
    # ---- moments
    ref, got = c["moments"], run_moments(c["table"], lat_sizes, c["rows"])
    assert got["min"].tobytes() == ref["min"].tobytes() and got["max"].tobytes() == ref["max"].tobytes(), what
    e32 = R.moment_ratios(c["moments32"], ref)
    ratio = R.moment_ratios(got, ref)
    print("%s: err / tol kernel %s | fp32 restatement %s" % (what, {k: round(v, 4) for k, v in ratio.items()},
                                                              {k: round(v, 4) for k, v in e32.items()}))
    for k in ratio:
        assert e32[k] <= R.CAP, (what, k, "the case itself is out of the rule's range", e32[k])
        assert ratio[k] <= R.bound(e32[k]), (what, k, ratio[k], e32[k])
    again = run_moments(c["table"], lat_sizes, c["rows"])
    assert all(again[k].tobytes() == got[k].tobytes() for k in MOMENT_KEYS), what + ": second run"
    if S == 1:
        assert not got["var"].any() and not got["cov"].any() and not got["factor_var"].any()
    return ratio


# ---- 1. kernel parity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lat_sizes,D,n_bins,family", R.CASES)
def test_counts_and_moments_vs_fp64(lat_sizes, D, n_bins, family):
    for S in R.SELECTIONS:
        assert_case(lat_sizes, D, n_bins, family, S)


@pytest.mark.parametrize("lat_sizes,D,n_bins,family,S", R.switch_cases(_infolib))
def test_counts_and_moments_on_both_sides_of_every_switch(lat_sizes, D, n_bins, family, S):
    assert_case(lat_sizes, D, n_bins, family, S)


def test_selected_rows_keep_their_own_factor_values():
    """The factor value comes from the row NUMBER, not from the position in `rows`: a selection of one value of factor 0."""
    lat = (3, 4, 5)
    table = R.make_table(lat, 3, "disent")
    rows = np.arange(20, 40)[::-1].copy()                        # factor 0 = 1 throughout, out of order
    counts = run_hist(table, lat, R.joint_counts(table, lat, 20, rows)[1], rows)
    assert np.array_equal(counts, R.joint_counts(table, lat, 20, rows)[0])
    block = R.blocks_of(counts[0], lat, 20)[0]
    assert block[:, 1].sum() == 20 and block.sum() == 20
    got = run_moments(table, lat, rows)
    assert got["factor_mean"][0] == 1.0 and got["factor_var"][0] == 0.0 and got["factor_mean"][2] == 2.0


# ---- 2. memory contract --------------------------------------------------------------------------------------------------------
def _info_call(name):
    def fn(args):
        _infolib.call(name, *[a.ptr if isinstance(a, Guarded) else a for a in args])
    return fn


# small; odd (17 columns, 7 bins, 65 selected rows); the factor with more values than the LDS histogram holds
CONTRACT_SHAPES = [((3, 4, 5), 3, 20, None), ((2, 3, 6, 40), 17, 7, 65), ((1000, 3), 10, 20, None)]


@pytest.mark.parametrize("lat_sizes,D,n_bins,S", CONTRACT_SHAPES)
def test_memory_contract_moments(lat_sizes, D, n_bins, S):
    """Guards untouched, inputs unchanged, every output element written, bits equal to the run on plain tensors whatever the
    workspace and the surroundings hold (NaN at 256-byte alignment; -1e30 at the weakest alignment promised: the element's own)."""
    c = R.case(lat_sizes, D, n_bins, "gauss", S)
    N, K = c["table"].shape[0], len(lat_sizes)
    n_sel = N if S is None else S
    nws = _infolib.lib().dvae_info_moments_ws_floats(N, D, K, n_sel)

    def build(al):
        rows = None if S is None else al.inp("rows", c["rows"].astype(np.int64), align=8)
        return [al.inp("table", c["table"], align=4), rows, al.inp("lat_sizes", np.array(lat_sizes, dtype=np.int32), align=4), N, D, K,
                n_sel, al.ws("ws", (nws,), align=4), al.out("col_min", (D,), align=4), al.out("col_max", (D,), align=4),
                al.out("col_mean", (D,), align=4), al.out("col_var", (D,), align=4), al.out("cov_zv", (D, K), align=4),
                al.out("factor_mean", (K,), align=4), al.out("factor_var", (K,), align=4), stream()]
    run_contract("dvae_info_moments", build, fn=_info_call("dvae_info_moments"))


@pytest.mark.parametrize("lat_sizes,D,n_bins,S", CONTRACT_SHAPES)
def test_memory_contract_joint_hist(lat_sizes, D, n_bins, S):
    c = R.case(lat_sizes, D, n_bins, "gauss", S)
    N, K, total = c["table"].shape[0], len(lat_sizes), sum(lat_sizes)
    n_sel = N if S is None else S

    def build(al):
        rows = None if S is None else al.inp("rows", c["rows"].astype(np.int64), align=8)
        return [al.inp("table", c["table"], align=4), rows, al.inp("lat_sizes", np.array(lat_sizes, dtype=np.int32), align=4),
                al.inp("edges", c["edges"], align=4), N, D, K, n_sel, n_bins, total, al.ws("ws", (1,), align=4),
                al.out("counts", (D, n_bins * total), dtype=torch.int32, align=4), stream()]
    runs = run_contract("dvae_info_joint_hist", build, fn=_info_call("dvae_info_joint_hist"))
    assert np.array_equal(runs[0].args[-1].t.cpu().numpy(), c["counts"])


# ---- 3. the scores from a table ------------------------------------------------------------------------------------------------
def sap_tolerance(ref_mom):
    """The moment tolerances carried through sap = cov^2 / (var_z var_v), first order plus the square of the covariance's."""
    tol = R.moment_tolerances(ref_mom)
    vz, vv, c = ref_mom["var"][:, None], ref_mom["factor_var"][None, :], ref_mom["cov"]
    live = (ref_mom["var"] > 1e-12)[:, None]
    vz = np.where(live, vz, 1.0)
    sap = c ** 2 / (vz * vv)
    out = (2 * np.abs(c) * tol["cov"] + tol["cov"] ** 2) / (vz * vv) + sap * (tol["var"][:, None] / vz + tol["factor_var"][None, :] / vv)
    return np.where(live, out, 0.0) + 1e-15


def assert_scores(got, ref, ref_mom):
    assert set(got) == {"mig_discrete", "modularity", "sap_continuous", "sap_matrix", "mutual_information", "factor_entropy",
                        "n_samples", "n_bins"}
    assert (got["n_samples"], got["n_bins"]) == (ref["n_samples"], ref["n_bins"])
    for key in ("mig_discrete", "modularity", "mutual_information", "factor_entropy"):       # exact counts, fp64 on the host
        assert np.abs(got[key] - ref[key]).max() <= 1e-12, key
    tol = sap_tolerance(ref_mom)
    err = np.abs(got["sap_matrix"] - ref["sap_matrix"])
    print("sap_matrix: worst err / tol %.3f" % (err / tol).max())
    assert (err <= tol).all()
    assert abs(got["sap_continuous"] - ref["sap_continuous"]) <= 2 * tol.max()
    assert isinstance(got["mig_discrete"], float) and isinstance(got["sap_matrix"], np.ndarray) and isinstance(got["n_samples"], int)


@pytest.mark.parametrize("lat_sizes,D,n_bins,kind", [((3, 4, 5), 5, 20, "ideal"), ((3, 4, 5), 5, 20, "rotated"),
                                                      ((3, 6, 40, 32), 10, 20, "gauss"), ((1000, 3), 3, 64, "disent")])
def test_scores_from_table_vs_fp64(lat_sizes, D, n_bins, kind):
    table = {"ideal": R.ideal_table, "rotated": R.rotated_table}[kind](lat_sizes, D) if kind in ("ideal", "rotated") else \
        R.make_table(lat_sizes, D, kind)
    got = information_scores_from_table(torch.from_numpy(table).to(DEV), lat_sizes, n_bins=n_bins)
    ref = R.scores(table, lat_sizes, n_bins)
    print(kind, {k: v for k, v in got.items() if not isinstance(v, np.ndarray)})
    assert_scores(got, ref, R.moments(table, lat_sizes))
    if kind == "ideal":
        assert abs(got["mig_discrete"] - 1) < 1e-12 and abs(got["sap_continuous"] - 1) < 1e-6 and abs(got["modularity"] - 3 / 5) < 1e-12
    if kind == "rotated":
        ideal = information_scores_from_table(torch.from_numpy(R.ideal_table(lat_sizes, D)).to(DEV), lat_sizes, n_bins=n_bins)
        assert all(got[k] < ideal[k] for k in ("mig_discrete", "modularity", "sap_continuous"))
    rows = np.random.default_rng(3).integers(0, table.shape[0], size=777)                     # an injected selection
    got = information_scores_from_table(torch.from_numpy(table).to(DEV), lat_sizes, n_bins=n_bins, rows=rows)
    assert_scores(got, R.scores(table, lat_sizes, n_bins, rows), R.moments(table, lat_sizes, rows))


def test_scores_from_table_seeds_and_random_states():
    lat = (2, 3, 6, 40)
    table = torch.from_numpy(R.make_table(lat, 10, "gauss")).to(DEV)      # (independent columns: every estimate follows the sample)
    cpu0, dev0 = torch.get_rng_state(), torch.cuda.get_rng_state()
    a, b, c = (information_scores_from_table(table, lat, n_samples=500, seed=s) for s in (3, 3, 4))
    assert torch.equal(torch.get_rng_state(), cpu0) and torch.equal(torch.cuda.get_rng_state(), dev0)
    assert a["n_samples"] == 500 and a["mig_discrete"] == b["mig_discrete"] and a["mig_discrete"] != c["mig_discrete"]
    assert not np.array_equal(a["mutual_information"], c["mutual_information"])
    assert all(np.array_equal(a[k], b[k]) for k in a)
    gen = torch.Generator(device=DEV).manual_seed(3)                # the documented draw: randperm(N)[:n_samples]
    rows = torch.randperm(1440, generator=gen, device=DEV)[:500]
    d = information_scores_from_table(table, lat, rows=rows)
    assert all(np.array_equal(a[k], d[k]) for k in a)
    assert_scores(a, R.scores(table.cpu().numpy(), lat, 20, rows.cpu().numpy()), R.moments(table.cpu().numpy(), lat, rows.cpu().numpy()))
    with pytest.raises(ValueError, match="no entropy"):            # one selected row: no factor varies
        information_scores_from_table(table, lat, rows=[5])
    bad = table.clone()
    bad[7, 2] = float("inf")
    with pytest.raises(ValueError, match="NaN or an infinity"):
        information_scores_from_table(bad, lat)


# ---- 4. Evaluator end to end ---------------------------------------------------------------------------------------------------
class _FactorData:
    """tiny data set with known factors, iterated in factor order (what compute_information_scores requires)."""
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
    torch.manual_seed(3)
    model = init_specific_model("Burgess", img, 10)
    loss_f = get_loss_f("btcvae", device=torch.device(DEV), n_data=N, rec_dist="bernoulli", reg_anneal=0, btcvae_A=1, btcvae_B=6,
                        btcvae_G=1)
    images = torch.rand((N,) + img, generator=torch.Generator().manual_seed(4))
    loader = _Loader(images, 16)
    ev = Evaluator(model, loss_f, device=torch.device(DEV), logger=logging.getLogger("i"), save_dir=str(tmp_path),
                   is_progress_bar=False)
    model.train()
    got = ev.compute_information_scores(loader, n_bins=8)
    assert model.training
    model.eval()
    with torch.no_grad():
        mean, _ = model.encoder(images.to(DEV))
    model.train()
    table = mean.cpu().numpy()
    assert_scores(got, R.scores(table, lat, 8), R.moments(table, lat))
    assert got["n_samples"] == N and got["mutual_information"].shape == (10, 3) and 0.0 <= got["modularity"] <= 1.0
    part = ev.compute_information_scores(loader, n_samples=40, seed=1)
    assert part["n_samples"] == 40 and part["n_bins"] == 20 and part["mutual_information"].shape == (10, 3)
    # Evaluator.__call__: with its defaults exactly the file it wrote before; the new one only on request, without matrices
    ev(loader)
    assert sorted(os.listdir(tmp_path)) == ["test_losses.log"]
    assert ev(loader, is_losses=False, is_information=True) == (None, None)
    assert sorted(os.listdir(tmp_path)) == ["information_scores.log", "test_losses.log"]
    logged = json.load(open(tmp_path / "information_scores.log"))
    assert set(logged) == {"mig_discrete", "modularity", "sap_continuous", "factor_entropy", "n_samples", "n_bins"}
    assert logged["n_samples"] == N and logged["n_bins"] == 20 and len(logged["factor_entropy"]) == 3
    full = ev.compute_information_scores(loader)
    assert logged["mig_discrete"] == full["mig_discrete"] and logged["modularity"] == full["modularity"]
    assert model.training

    class _NoFactors:
        dataset = [0, 1, 2, 3]
    with pytest.raises(ValueError, match="known true factors"):
        ev.compute_information_scores(_NoFactors())
    assert _lib.lib().dvae_version() == 109
