"""-m gpu: the posterior mass library (lib/ext/libdvae_mass_hip.so, csrc/posterior_mass.hip;
Evaluator.compute_interpretability_scores) against the fp64 restatement of tests/mass_ref.py.

The switches of the launcher, and the case on each side of each (mass_ref.cases):
  * waves per workgroup, ceil(n_bins / 63): n_bins 1, 2, 63 -> one (63: the wave's last lane holds the +inf edge); 64, 65, 100 -> two
    (64: the second wave owns one bin); 128, 129 -> three; MAX_BINS = 256 -> five;
  * trips of 64 rows: S = 1 and N = 6, 24 -> one; S = 65 -> a second trip of one row; N = 720 -> whole and ragged trips;
  * chunks: S = 257 -> two; S = BLOCK_ROWS * MAX_CHUNKS - 1, that, and one more: 128 chunks, the last one short / all of them full /
    the chunks grow to BLOCK_ROWS + 1 rows (D = 1, n_bins = 4);
  * column groups: lat_sizes (40, 38) at MAX_BINS fill the LDS accumulators of one workgroup, (40, 39) take two groups, the second
    of which starts inside factor 1.

Tolerance.  Per cell B = n_v (2 U_REF + 3) 2^-53, n_v the number of selected rows that carry the cell's factor value
(mass_ref.cell_bound; U_REF is math.erfc's own error, measured by tests/test_mass_host.py); the device passes at 4 B -- the 4 covers
a device erfc a few ulp looser than libm's, after the project's max(1, 4 e) precedent, and was fixed before the first run.  The sum
over the bins of a column is held to n_bins * 4 B of n_v.  Every ratio is printed."""
import json
import logging
import os

import numpy as np
import pytest
import torch

import mass_ref as R
from gpu_util import DEV, stream
from guard_util import Guarded, run_contract
from disvae_amd import _masslib, Evaluator, interpretability_scores_from_mass, interpretability_scores_from_table

pytestmark = pytest.mark.gpu
CASES = R.cases(_masslib.MAX_BINS, _masslib.BLOCK_ROWS, _masslib.MAX_CHUNKS, _masslib.LDS_DOUBLES)


def _id(c):
    return "%s-D%d-nb%d-%s-S%s" % ("x".join(map(str, c[0])), c[1], c[2], c[3], c[4])


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype).contiguous()


def run_mass(lat_sizes, n_bins, c, st=None, fill=float("nan")):
    """dvae_mass_joint on a poisoned workspace and output -> mass [D, n_bins * sum(lat_sizes)] as fp64 numpy."""
    mean, logvar, rows = c["mean"], c["logvar"], c["rows"]
    (N, D), K, sums = mean.shape, len(lat_sizes), sum(lat_sizes)
    assert logvar.shape == (N, D) and N == int(np.prod(lat_sizes))             # the kernels trust these sizes
    assert rows is None or (rows.min() >= 0 and rows.max() < N)
    S = N if rows is None else len(rows)
    need = _masslib.lib().dvae_mass_ws_doubles(N, D, K, S, n_bins, sums)
    assert need == _masslib.ws_doubles(N, D, K, S, n_bins, sums) > 0
    md, ld, sd = _dev(mean), _dev(logvar), _dev(np.array(lat_sizes), torch.int32)
    rd = None if rows is None else _dev(rows, torch.int64)
    ed = _dev(R.edges(n_bins), torch.float64) if n_bins > 1 else None
    ws = torch.full((need,), fill, dtype=torch.float64, device=DEV)
    mass = torch.full((D, n_bins * sums), fill, dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    _masslib.call("dvae_mass_joint", md.data_ptr(), ld.data_ptr(), None if rd is None else rd.data_ptr(), sd.data_ptr(),
                  None if ed is None else ed.data_ptr(), N, D, K, S, n_bins, sums, ws.data_ptr(), mass.data_ptr(),
                  stream() if st is None else st)
    torch.cuda.synchronize()
    return mass.cpu().numpy()


# ---- 1. the mass table against the restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_mass_vs_fp64(case):
    lat_sizes, D, n_bins, family, S = case
    c = R.case(*case)
    got = run_mass(lat_sizes, n_bins, c)
    ref, B = c["mass"], R.cell_bound(c["cells"])
    assert got.shape == ref.shape and np.isfinite(got).all() and (got >= 0).all()
    err = np.abs(got - ref)
    live = B > 0
    ratio = float((err[live] / B[live]).max())
    # the masses of a row sum to 1: a column's bins sum to the rows that carry its value
    worst_sum, start = 0.0, 0
    for k, size in enumerate(lat_sizes):
        sums = got[:, start * n_bins:(start + size) * n_bins].reshape(D, n_bins, size).sum(axis=1)        # [D, size]
        n_v = c["n_v"][start:start + size].astype(np.float64)
        bound = n_bins * 4 * R.cell_bound(n_v)
        assert (np.abs(sums - n_v)[:, n_v == 0] == 0).all()
        worst_sum = max(worst_sum, float((np.abs(sums - n_v)[:, n_v > 0] / bound[n_v > 0]).max()))
        start += size
    print("%s: worst cell error %.3f B (passes at 4 B); worst column sum %.3f of its bound" % (_id(case), ratio, worst_sum))
    assert (got[~live] == 0).all()                                            # a value no selected row carries: exactly nothing
    assert ratio <= 4.0, (_id(case), ratio)
    assert worst_sum <= 1.0, (_id(case), worst_sum)
    assert c["S"] == (c["N"] if S is None else S) and abs(got[0, :n_bins * lat_sizes[0]].sum() - c["S"]) <= 1e-9 * c["S"]


# ---- 2. determinism, memory ---------------------------------------------------------------------------------------------------------
DET_CASES = [c for c in CASES if (c[0], c[2], c[4]) in ((R.GRID, 65, 1000), ((40, CASES[-4][0][1]), _masslib.MAX_BINS, 300),
                                                        ((4, 3, 2), 4, _masslib.BLOCK_ROWS * _masslib.MAX_CHUNKS + 1))]


@pytest.mark.parametrize("case", DET_CASES, ids=_id)
def test_same_bits_twice_and_on_a_second_stream_with_poisoned_buffers(case):
    assert len(DET_CASES) == 3
    lat_sizes, D, n_bins, family, S = case
    c = R.case(*case)
    a = run_mass(lat_sizes, n_bins, c, fill=float("nan"))
    b = run_mass(lat_sizes, n_bins, c, fill=0.0)
    assert not np.isnan(a).any() and a.tobytes() == b.tobytes()              # every element is written, whatever was there
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d = run_mass(lat_sizes, n_bins, c, st=side.cuda_stream, fill=-1e300)
    assert a.tobytes() == d.tobytes()


def _mass_call(args):
    _masslib.call("dvae_mass_joint", *[a.ptr if isinstance(a, Guarded) else a for a in args])


CONTRACT_CASES = [((3, 2), 1, 1, "broad", 1), ((4, 3, 2), 3, 65, "broad", None), (R.GRID, 3, 63, "tiny", 65), CASES[-4]]


@pytest.mark.parametrize("case", CONTRACT_CASES, ids=_id)
def test_memory_contract(case):
    """Guards untouched, inputs unchanged, every output element written, bits equal to the run on plain tensors whatever the
    workspace and the surroundings hold (NaN at 256-byte alignment; -1e30 at the weakest alignment promised: the element's own)."""
    assert case in CASES
    lat_sizes, D, n_bins, family, S = case
    c = R.case(*case)
    N, K, sums = c["N"], len(lat_sizes), sum(lat_sizes)
    nws = _masslib.ws_doubles(N, D, K, c["S"], n_bins, sums)
    edges = R.edges(n_bins) if n_bins > 1 else np.zeros(1)                    # (one bin: not read)

    def build(al):
        return [al.inp("mean", c["mean"], align=4), al.inp("logvar", c["logvar"], align=4),
                None if c["rows"] is None else al.inp("rows", torch.from_numpy(c["rows"]), align=8),
                al.inp("lat_sizes", torch.tensor(lat_sizes, dtype=torch.int32), align=4),
                al.inp("edges", torch.from_numpy(edges), align=8, dtype=torch.float64), N, D, K, c["S"], n_bins, sums,
                al.ws("ws", (nws,), dtype=torch.float64, align=8), al.out("mass", (D, n_bins * sums), dtype=torch.float64, align=8), stream()]
    runs = run_contract("dvae_mass_joint", build, fn=_mass_call)
    got = runs[0].args[-1].t.cpu().numpy()
    assert (np.abs(got - c["mass"]) <= 4 * R.cell_bound(c["cells"])).all()


def test_a_layout_that_is_not_the_devices_leaves_every_element_zero():
    case = ((4, 3, 2), 3, 65, "broad", None)
    c = dict(R.case(*case))
    md, ld = _dev(c["mean"]), _dev(c["logvar"])
    sd, ed = _dev(np.array([4, 3, 3]), torch.int32), _dev(R.edges(65), torch.float64)      # sums to 10, the caller says 9
    ws = torch.full((_masslib.ws_doubles(24, 3, 3, 24, 65, 9),), float("nan"), dtype=torch.float64, device=DEV)
    mass = torch.full((3, 65 * 9), float("nan"), dtype=torch.float64, device=DEV)
    _masslib.call("dvae_mass_joint", md.data_ptr(), ld.data_ptr(), None, sd.data_ptr(), ed.data_ptr(), 24, 3, 3, 24, 65, 9, ws.data_ptr(),
                  mass.data_ptr(), stream())
    torch.cuda.synchronize()
    assert (mass == 0).all()


# ---- 3. the scores from the device's table against the scores from the reference's -----------------------------------------------
SCORE_CASES = [c for c in CASES if c[4] is None and c[2] >= 63 and c[0] != (3, 2)] + [(R.GRID, 10, 65, "sharp", 1000)]


@pytest.mark.parametrize("case", SCORE_CASES, ids=_id)
def test_scores_from_the_device_table(case):
    lat_sizes, D, n_bins, family, S = case
    c = R.case(*case)
    got = interpretability_scores_from_mass(run_mass(lat_sizes, n_bins, c), lat_sizes, n_bins)
    ref = R.scores(c["mass"], lat_sizes, n_bins)
    bound = R.score_bound(c["mass"], 4 * R.cell_bound(c["cells"]), lat_sizes, n_bins)      # sum over the cells of |log P + 1| 4 B / S
    worst = max(float(np.abs(np.asarray(got[k], dtype=np.float64) - ref[k]).max()) for k in ref if k != "best_latent")
    print("%s: worst score error %.3g, bound %.3g" % (_id(case), worst, bound))
    # (the bound: below 1e-10 for the tables of three latents but the "far" one, whose cells of 1e-300 have |log P| = 700: 2.6e-9)
    assert bound < 1e-8
    assert worst <= bound, (_id(case), worst, bound)
    assert got["best_latent"].tolist() == ref["best_latent"].tolist() and got["n_samples"] == c["S"]


def test_from_table_selection_seed_and_errors():
    mean, logvar = R.ideal_table()
    md, ld = _dev(mean), _dev(logvar)
    cpu0, dev0 = torch.get_rng_state(), torch.cuda.get_rng_state()
    full = interpretability_scores_from_table(md, ld, R.GRID)
    a = interpretability_scores_from_table(md, ld, R.GRID, n_samples=500, seed=3)
    b = interpretability_scores_from_table(md, ld, R.GRID, n_samples=500, seed=3)
    c = interpretability_scores_from_table(md, ld, R.GRID, n_samples=500, seed=4)
    assert torch.equal(torch.get_rng_state(), cpu0) and torch.equal(torch.cuda.get_rng_state(), dev0)
    assert full["n_samples"] == 720 and full["n_bins"] == 100 and a["n_samples"] == 500
    assert a["rmig"] == b["rmig"] and np.array_equal(a["mutual_information"], b["mutual_information"]) and a["rmig"] != c["rmig"]
    rows = np.array([5, 5, 700, 33, 0, 719, 360, 5])
    got = interpretability_scores_from_table(md, ld, R.GRID, n_bins=7, z_range=(-3.0, 2.0), rows=rows)
    want = R.scores(R.mass_table(mean, logvar, R.GRID, 7, z_range=(-3.0, 2.0), rows=rows)[0], R.GRID, 7)
    assert got["n_samples"] == 8 and got["n_bins"] == 7
    for k in R.SCALAR_SCORES:
        assert got[k] == pytest.approx(want[k], abs=1e-12), k
    with pytest.raises(ValueError, match="no entropy"):                      # one selected row: no factor varies
        interpretability_scores_from_table(md, ld, R.GRID, rows=[5])
    bad = ld.clone()
    bad[7, 2] = float("inf")
    with pytest.raises(ValueError, match="NaN or an infinity"):
        interpretability_scores_from_table(md, bad, R.GRID)


# ---- 4. Evaluator end to end ----------------------------------------------------------------------------------------------------------
class _TableModel(torch.nn.Module):
    """A model whose encoder looks q(z|x) up in a table: image x is its row number."""

    def __init__(self, mean, logvar):
        super().__init__()
        self.latent_dim = mean.shape[1]
        self.register_buffer("mean", torch.from_numpy(np.ascontiguousarray(mean)))
        self.register_buffer("logvar", torch.from_numpy(np.ascontiguousarray(logvar)))
        self.modes = []

    def encoder(self, x):
        self.modes.append(self.training)
        idx = x.view(-1).long()
        return self.mean[idx], self.logvar[idx]


class _Factors:
    lat_sizes, lat_names = np.array(R.GRID), tuple("abcde")

    def __len__(self):
        return 720


class _Loader:
    dataset = _Factors()

    def __iter__(self):
        for lo in range(0, 720, 100):
            yield torch.arange(lo, min(lo + 100, 720), dtype=torch.float32).view(-1, 1), None


def _setup(table, tmp_path):
    model = _TableModel(*table).train()
    ev = Evaluator(model, None, device=torch.device(DEV), logger=logging.getLogger("mass"), save_dir=str(tmp_path), is_progress_bar=False)
    return model, ev


def test_evaluator_on_the_ideal_and_the_rotated_table(tmp_path):
    model, ev = _setup(R.ideal_table(), tmp_path)
    ideal = ev.compute_interpretability_scores(_Loader())
    assert model.training and model.modes == [False] * 8                     # encoded in eval mode, mode restored
    print("ideal: %s" % {k: round(ideal[k], 4) for k in R.SCALAR_SCORES})
    assert ideal["rmig_norm"] >= 0.99 and ideal["jemmig_norm"] >= 0.9
    assert ideal["best_latent"].tolist() == [0, 1, 2, 3, 4] and ideal["n_samples"] == 720 and ideal["n_bins"] == 100
    assert ideal["mutual_information"].shape == ideal["joint_entropy"].shape == (7, 5)
    want = R.scores(R.mass_table(*R.ideal_table(), R.GRID, 100)[0], R.GRID, 100)
    for k in R.SCALAR_SCORES:
        assert ideal[k] == pytest.approx(want[k], abs=1e-10), k
    rmodel, rev = _setup(R.rotated_table(), tmp_path)
    rotated = rev.compute_interpretability_scores(_Loader())
    print("rotated: %s" % {k: round(rotated[k], 4) for k in R.SCALAR_SCORES})
    assert rotated["rmig_norm"] <= 0.5 and rotated["jemmig_norm"] <= 0.35
    part = ev.compute_interpretability_scores(_Loader(), n_samples=300, n_bins=20, z_range=(-3.0, 3.0), seed=1)
    assert part["n_samples"] == 300 and part["n_bins"] == 20 and part["rmig_norm"] >= 0.9
    # Evaluator.__call__: the file only on request, without the [D, K] matrices; the return value the reference's
    assert ev(_Loader(), is_losses=False) == (None, None) and os.listdir(tmp_path) == []
    assert ev(_Loader(), is_losses=False, is_interpretability=True) == (None, None)
    assert os.listdir(tmp_path) == ["interpretability_scores.log"]
    logged = json.load(open(tmp_path / "interpretability_scores.log"))
    assert set(logged) == set(ideal) - {"mutual_information", "joint_entropy"}
    assert logged["rmig_norm"] == ideal["rmig_norm"] and logged["jemmig_per_factor"] == ideal["jemmig_per_factor"].tolist()
    ev(_Loader(), is_losses=False, is_interpretability=True, interpretability_args=dict(n_bins=20, n_samples=300, seed=1, z_range=(-3.0, 3.0)))
    assert json.load(open(tmp_path / "interpretability_scores.log"))["rmig_norm"] == part["rmig_norm"]
    assert model.training and not any(model.modes)

    class _NoFactors:
        dataset = [0, 1, 2, 3]
    with pytest.raises(ValueError, match="Dataset needs to have known true factors of variations to compute the metric"):
        ev.compute_interpretability_scores(_NoFactors())
