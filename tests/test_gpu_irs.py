"""-m gpu: the group-mean and segmented-selection kernels (libdvae_irs_hip.so, csrc/factor_irs.hip), irs_from_table and
Evaluator.compute_irs against the fp64 restatement of tests/irs_ref.py -- every count exactly, every mean inside the accumulation
bound 0.5 ulp32 (1 + 1e-6) + n_g 2^-52 max|x - x_0|, every order statistic bit for bit against numpy.sort, on both sides of every
dispatch macro of include/dvae_irs_hip.h (a second piece of columns, one workgroup / two, the grid cap, one slice of groups /
two, the most groups taken), on tables built to break a radix select, the memory contract of the two launching entry points, and
the score end to end.

Measured on the MI355X, worst over all cases below: see DESIGN.md section 2."""
import json
import logging
import os

import numpy as np
import pytest
import torch

import info_ref as I
import irs_ref as R
from gpu_util import DEV, dev, keep, stream
from guard_util import Guarded, run_contract
from disvae_amd import _irslib, _lib, Evaluator
from disvae_amd.evaluate import irs_from_table
from disvae_amd.models.losses import get_loss_f
from disvae_amd.models.vae import init_specific_model

pytestmark = pytest.mark.gpu


def _layout(table, lat_sizes, factor_bins, rows):
    N, D = table.shape
    if rows is not None:
        assert 0 <= rows.min() and rows.max() < N                  # the kernels trust the rows
    gmap, n_groups = R.group_layout(lat_sizes, factor_bins)
    t = dev(torch.from_numpy(table))
    r = None if rows is None else keep(torch.from_numpy(rows.astype(np.int64)).to(DEV))
    sizes = keep(torch.tensor(lat_sizes, dtype=torch.int32, device=DEV))
    m = keep(torch.from_numpy(gmap).to(DEV))
    g = keep(torch.tensor(n_groups, dtype=torch.int32, device=DEV))
    total = 1 + sum(n_groups)
    ptrs = (t.data_ptr(), None if r is None else r.data_ptr(), sizes.data_ptr(), m.data_ptr(), g.data_ptr())
    return ptrs, (N, D, len(lat_sizes), (N if rows is None else len(rows)), sum(lat_sizes), total, max(n_groups))


def run_means(table, lat_sizes, factor_bins, rows=None):
    ptrs, sizes = _layout(table, lat_sizes, factor_bins, rows)
    N, D, K, S, _sum, total, _most = sizes
    need = _irslib.lib().dvae_irs_group_means_ws_floats(N, D, K, S, total)
    assert need > 0
    ws = keep(torch.full((need,), float("nan"), device=DEV))
    counts = torch.full((total,), -7, dtype=torch.int32, device=DEV)
    means = torch.full((total, D), float("nan"), device=DEV)
    _irslib.call("dvae_irs_group_means", *ptrs, *sizes, ws.data_ptr(), counts.data_ptr(), means.data_ptr(), stream())
    return counts.cpu().numpy(), means.cpu().numpy()


def run_stats(table, lat_sizes, factor_bins, centres, ranks, rows=None):
    ptrs, sizes = _layout(table, lat_sizes, factor_bins, rows)
    N, D, K, S, _sum, total, _most = sizes
    assert centres.shape == (total, D) and centres.dtype == np.float32 and len(ranks) == total
    need = _irslib.lib().dvae_irs_group_order_stats_ws_floats(N, D, K, S, total)
    assert need > 0
    ws = keep(torch.full((need,), float("nan"), device=DEV))
    c = dev(torch.from_numpy(centres))
    k = keep(torch.from_numpy(np.asarray(ranks).astype(np.int32)).to(DEV))
    out = [torch.full((total, D), float("nan"), device=DEV) for _ in range(3)]
    _irslib.call("dvae_irs_group_order_stats", *ptrs, c.data_ptr(), k.data_ptr(), *sizes, ws.data_ptr(), *[o.data_ptr() for o in out],
                 stream())
    return [o.cpu().numpy() for o in out]


def assert_order_stats(table, lat_sizes, factor_bins, centres, rank_sets, rows, what):
    """stat_lo, stat_hi and dev_max against numpy.sort, bit for bit, for every set of ranks; the first set twice."""
    devs = R.sorted_deviations(table, lat_sizes, factor_bins, centres, rows)
    for i, (name, ranks) in enumerate(rank_sets.items()):
        ref = R.order_stats(devs, ranks)
        got = run_stats(table, lat_sizes, factor_bins, centres, ranks, rows)
        for key, g, r in zip(("stat_lo", "stat_hi", "dev_max"), got, ref):
            assert g.dtype == np.float32 and g.tobytes() == r.tobytes(), (what, name, key, np.argwhere(g.view(np.uint32) != r.view(np.uint32))[:4])
        if i == 0:
            again = run_stats(table, lat_sizes, factor_bins, centres, ranks, rows)
            assert all(a.tobytes() == g.tobytes() for a, g in zip(again, got)), what + ": second run"


def assert_case(lat_sizes, D, family, factor_bins, S):
    c = R.case(lat_sizes, D, family, factor_bins, S)
    what = "lat %s D %d %s bins %s S %s" % (lat_sizes, D, family, factor_bins, S)
    # ---- counts and means
    counts, means = run_means(c["table"], lat_sizes, factor_bins, c["rows"])
    assert counts.dtype == np.int32 and np.array_equal(counts, c["counts"]), what
    tol = R.mean_tolerance(c["means"], c["counts"], c["span"])
    err = np.abs(means.astype(np.float64) - c["means"])
    ratio = float((err / tol).max())
    print("%s: worst mean error / bound %.4f" % (what, ratio))
    assert (err <= tol).all(), (what, ratio)
    assert not means[c["counts"] == 0].any()
    again = run_means(c["table"], lat_sizes, factor_bins, c["rows"])
    assert again[0].tobytes() == counts.tobytes() and again[1].tobytes() == means.tobytes(), what + ": second run"
    if family == "const":                                          # the sums are taken around the first row: exact
        assert (means[c["counts"] > 0] == c["table"][0]).all()
    # ---- order statistics
    assert_order_stats(c["table"], lat_sizes, factor_bins, c["centres"], R.rank_sets(c["counts"]), c["rows"], what)
    return ratio


# ---- 1. kernel parity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lat_sizes,D,family,factor_bins", R.CASES)
def test_counts_means_and_order_stats_vs_fp64(lat_sizes, D, family, factor_bins):
    for S in R.SELECTIONS:
        assert_case(lat_sizes, D, family, factor_bins, S)


@pytest.mark.parametrize("lat_sizes,D,family,factor_bins,S", R.switch_cases(_irslib))
def test_counts_means_and_order_stats_on_both_sides_of_every_switch(lat_sizes, D, family, factor_bins, S):
    assert_case(lat_sizes, D, family, factor_bins, S)


def test_more_groups_than_the_limit_are_refused():
    lat = (_irslib.MAX_GROUPS + 1, 2)
    table = I.make_table(lat, 2, "gauss")
    ptrs, sizes = _layout(table, lat, None, None)
    big = 1 << 20
    with pytest.raises(_lib.DvaeHipError, match="DVAE_IRS_MAX_GROUPS"):
        _irslib.call("dvae_irs_group_means", *ptrs, *sizes, big, big, big, stream())


# ---- 2. tables built to break a radix select -------------------------------------------------------------------------------------
def _adversarial():
    """name -> (table, lat_sizes, rows).  The centres are zeros, so the deviations are |x| itself."""
    rng = np.random.default_rng(11)
    lat = (2, 125)
    n = 250
    out = {}
    out["all equal"] = (np.full((n, 3), -1.5, dtype=np.float32), lat, None)
    zeros = np.zeros((n, 3), dtype=np.float32)
    zeros[::2] = -0.0                                              # |-0 - 0| must come out as +0
    out["all zero"] = (zeros, lat, None)
    mant = (1.0 + rng.permutation(n)[:, None] % 256 * 2.0 ** -23).astype(np.float32)          # differ in the lowest byte only
    out["lowest mantissa byte"] = (np.concatenate([mant, -mant[::-1]], axis=1), lat, None)
    expo = (2.0 ** (rng.permutation(n)[:, None].astype(np.float64) - 149.0)).astype(np.float32)  # 2^-149 (denormal) .. 2^100
    assert expo.min() == np.float32(2.0 ** -149) and expo.max() == np.float32(2.0 ** 100) and len(np.unique(expo)) == n
    out["exponent byte"] = (np.concatenate([expo, -expo[::-1]], axis=1), lat, None)
    runs = np.repeat(np.arange(1, 26), 10).astype(np.float32)[:, None]                          # 25 values, ten of each
    out["runs of equal values"] = (np.concatenate([runs, runs[rng.permutation(n)]], axis=1), lat, None)
    out["one-row groups"] = (I.make_table(lat, 3, "gauss"), lat, np.array([0, 1, 2, 3, 3, 130]))  # factor 0: 5 rows / 1 row
    out["empty groups"] = (I.make_table(lat, 3, "gauss"), lat, rng.integers(0, 120, size=300))    # factor 0 = 1 never occurs
    return out


@pytest.mark.parametrize("name", sorted(_adversarial()))
def test_order_stats_on_tables_built_to_break_a_radix_select(name):
    table, lat, rows = _adversarial()[name]
    for bins in (None, 20):
        masks, _ = R.group_masks(lat, bins, rows)
        counts = masks.sum(axis=1)
        centres = np.zeros((len(counts), table.shape[1]), dtype=np.float32)
        sets = R.rank_sets(counts)
        devs = R.sorted_deviations(table, lat, bins, centres, rows)
        # the rank + 1 element being the first of a new value (column 0), and the last of a run of equal values
        edge = [np.flatnonzero(np.diff(d[:, 0]) != 0) for d in devs]
        sets["before a new value"] = np.array([e[len(e) // 2] if len(e) else -1 for e in edge])
        sets["after a new value"] = np.array([e[len(e) // 2] + 1 if len(e) else -1 for e in edge])
        skip = sets["middle"].copy()
        skip[1::3] = -1                                            # every third group skipped: zeros, the neighbours intact
        skip[2::7] = counts[2::7]                                  # ... and a rank just past the end
        sets["skipped"] = skip
        assert_order_stats(table, lat, bins, centres, sets, rows, "%s, bins %s" % (name, bins))
        if name == "empty groups":
            assert counts[2] == 0 and (counts[1:] > 0).sum() > 3
        if name == "one-row groups":
            assert counts[2] == 1
    if name == "all zero":
        got = run_stats(table, lat, 20, centres, sets["last"], rows)
        assert all(not g.view(np.uint32).any() for g in got)     # +0 bit for bit, never -0


# ---- 3. memory contract --------------------------------------------------------------------------------------------------------
def _irs_call(name):
    def fn(args):
        _irslib.call(name, *[a.ptr if isinstance(a, Guarded) else a for a in args])
    return fn


# small; odd (17 columns, 65 selected rows, unbinned); a factor whose groups take five selection workgroups per chunk
CONTRACT_SHAPES = [((3, 4, 5), 3, 20, None), ((2, 3, 6, 20), 17, None, 65), ((183, 2), 3, None, None)]


def _contract_inputs(al, c, lat_sizes, S):
    rows = None if S is None else al.inp("rows", c["rows"].astype(np.int64), align=8)
    return [al.inp("table", c["table"], align=4), rows, al.inp("lat_sizes", np.array(lat_sizes, dtype=np.int32), align=4),
            al.inp("group_of_value", c["gmap"], align=4), al.inp("n_groups", np.array(c["n_groups"], dtype=np.int32), align=4)]


@pytest.mark.parametrize("lat_sizes,D,factor_bins,S", CONTRACT_SHAPES)
def test_memory_contract_group_means(lat_sizes, D, factor_bins, S):
    """Guards untouched, inputs unchanged, every output element written, bits equal to the run on plain tensors whatever the
    workspace and the surroundings hold (NaN at 256-byte alignment; -1e30 at the weakest alignment promised: the element's own)."""
    c = R.case(lat_sizes, D, "gauss", factor_bins, S)
    N, K, total = c["table"].shape[0], len(lat_sizes), 1 + sum(c["n_groups"])
    n_sel = N if S is None else S
    nws = _irslib.lib().dvae_irs_group_means_ws_floats(N, D, K, n_sel, total)

    def build(al):
        return _contract_inputs(al, c, lat_sizes, S) + [N, D, K, n_sel, sum(lat_sizes), total, max(c["n_groups"]),
                                                        al.ws("ws", (nws,), align=4), al.out("counts", (total,), dtype=torch.int32, align=4),
                                                        al.out("means", (total, D), align=4), stream()]
    runs = run_contract("dvae_irs_group_means", build, fn=_irs_call("dvae_irs_group_means"))
    assert np.array_equal(runs[0].args[-2].t.cpu().numpy(), c["counts"])


@pytest.mark.parametrize("lat_sizes,D,factor_bins,S", CONTRACT_SHAPES)
def test_memory_contract_group_order_stats(lat_sizes, D, factor_bins, S):
    c = R.case(lat_sizes, D, "gauss", factor_bins, S)
    N, K, total = c["table"].shape[0], len(lat_sizes), 1 + sum(c["n_groups"])
    n_sel = N if S is None else S
    nws = _irslib.lib().dvae_irs_group_order_stats_ws_floats(N, D, K, n_sel, total)
    ranks = R.rank_sets(c["counts"])["quantile"].astype(np.int32)
    ranks[1] = -1                                                  # a skipped group is written too

    def build(al):
        return _contract_inputs(al, c, lat_sizes, S) + [al.inp("centres", c["centres"], align=4), al.inp("rank", ranks, align=4), N, D, K,
                                                        n_sel, sum(lat_sizes), total, max(c["n_groups"]), al.ws("ws", (nws,), align=4),
                                                        al.out("stat_lo", (total, D), align=4), al.out("stat_hi", (total, D), align=4),
                                                        al.out("dev_max", (total, D), align=4), stream()]
    runs = run_contract("dvae_irs_group_order_stats", build, fn=_irs_call("dvae_irs_group_order_stats"))
    ref = R.order_stats(R.sorted_deviations(c["table"], lat_sizes, factor_bins, c["centres"], c["rows"]), ranks)
    for g, r in zip(runs[0].args[-3:], ref):
        assert g.t.cpu().numpy().tobytes() == r.tobytes()


def test_a_layout_that_is_not_the_devices_writes_zeros():
    """sum_sizes / total_groups that disagree with lat_sizes / n_groups: every output element 0, nothing else touched."""
    lat, D = (3, 4, 5), 3
    c = R.case(lat, D, "gauss", 20, None)
    ptrs, sizes = _layout(c["table"], lat, 20, None)
    N, D, K, S, total_values, total, most = sizes
    for wrong in ((N, D, K, S, total_values + 1, total, most), (N, D, K, S, total_values, total + 1, most), (N, D, K, S, total_values, total, most - 1)):
        T = wrong[5]
        ws = keep(torch.full((max(_irslib.lib().dvae_irs_group_means_ws_floats(N, D, K, S, T),
                                  _irslib.lib().dvae_irs_group_order_stats_ws_floats(N, D, K, S, T)),), float("nan"), device=DEV))
        counts = torch.full((T,), -7, dtype=torch.int32, device=DEV)
        outs = [torch.full((T, D), float("nan"), device=DEV) for _ in range(4)]
        _irslib.call("dvae_irs_group_means", *ptrs, *wrong, ws.data_ptr(), counts.data_ptr(), outs[0].data_ptr(), stream())
        centres = dev(torch.zeros(T, D))
        rank = keep(torch.zeros(T, dtype=torch.int32, device=DEV))
        _irslib.call("dvae_irs_group_order_stats", *ptrs, centres.data_ptr(), rank.data_ptr(), *wrong, ws.data_ptr(),
                     *[o.data_ptr() for o in outs[1:]], stream())
        assert not counts.cpu().numpy().any() and all(not o.cpu().numpy().view(np.uint32).any() for o in outs)


# ---- 4. the score from a table -------------------------------------------------------------------------------------------------
KEYS = {"IRS", "disentanglement_scores", "parents", "IRS_matrix", "max_deviations", "active", "n_groups", "n_samples", "diff_quantile",
        "factor_bins"}


def assert_irs(got, table, lat_sizes, factor_bins, q, rows, what):
    ref = R.irs(table, lat_sizes, q, factor_bins, rows)
    assert set(got) == KEYS
    assert got["n_samples"] == (table.shape[0] if rows is None else len(rows)) and got["diff_quantile"] == q
    assert got["factor_bins"] == factor_bins and got["n_groups"] == R.group_layout(lat_sizes, factor_bins)[1]
    assert isinstance(got["IRS"], float) and isinstance(got["IRS_matrix"], np.ndarray) and isinstance(got["n_samples"], int)
    assert np.array_equal(got["active"], ref["active"]), what
    if not ref["active"].any():
        assert got["IRS"] == 0.0 and got["IRS_matrix"].shape == (0, len(lat_sizes))
        return 0.0
    ratio = R.worst_ratio(got, ref, R.matrix_bound(table, ref))
    print("%s: IRS %.6f (fp64 %.6f), worst error / bound %.4f" % (what, got["IRS"], ref["IRS"], ratio))
    assert ratio <= 1.0, (what, ratio)
    return ratio


@pytest.mark.parametrize("kind,lat_sizes,D,factor_bins,q,S", R.END_TO_END)
def test_irs_from_table_vs_fp64(kind, lat_sizes, D, factor_bins, q, S):
    """Every entry of IRS_matrix, disentanglement_scores and IRS within 4 * 2^-24 max|table| / max_deviations[d] of the fp64
    restatement (precondition: tests/test_irs_host.py); ideal tables give exactly 1.0."""
    table = R.end_to_end_table(kind, lat_sizes, D)
    rows = R.rows_of(table.shape[0], D, S)
    got = irs_from_table(torch.from_numpy(table).to(DEV), lat_sizes, diff_quantile=q, factor_bins=factor_bins, rows=rows)
    assert_irs(got, table, lat_sizes, factor_bins, q, rows, "%s %s D %d" % (kind, lat_sizes, D))
    if kind == "ideal":
        assert got["IRS"] == 1.0 and (got["disentanglement_scores"] == 1.0).all() and list(got["parents"]) == list(range(len(lat_sizes)))
    if kind == "rotated":
        assert got["IRS"] < 1.0
    if kind == "const":
        assert got["IRS"] == 0.0 and not got["active"].any() and not got["max_deviations"].any()


def test_irs_from_table_seeds_and_random_states():
    lat = (2, 3, 6, 20)
    host = I.make_table(lat, 10, "gauss")
    table = torch.from_numpy(host).to(DEV)
    cpu0, dev0 = torch.get_rng_state(), torch.cuda.get_rng_state()
    a, b, c = (irs_from_table(table, lat, n_samples=300, seed=s) for s in (3, 3, 4))
    assert torch.equal(torch.get_rng_state(), cpu0) and torch.equal(torch.cuda.get_rng_state(), dev0)
    assert a["n_samples"] == 300 and a["IRS"] == b["IRS"] and a["IRS"] != c["IRS"]
    assert all(np.array_equal(a[k], b[k]) for k in a)
    gen = torch.Generator(device=DEV).manual_seed(3)                # the documented draw: randperm(N)[:n_samples]
    rows = torch.randperm(720, generator=gen, device=DEV)[:300]
    d = irs_from_table(table, lat, rows=rows)
    assert all(np.array_equal(a[k], d[k]) for k in a)
    assert_irs(a, host, lat, 20, 0.99, rows.cpu().numpy(), "300 drawn rows")
    bad = table.clone()
    bad[7, 2] = float("inf")
    with pytest.raises(ValueError, match="NaN or an infinity"):
        irs_from_table(bad, lat)


# ---- 5. Evaluator end to end ---------------------------------------------------------------------------------------------------
class _FactorData:
    """tiny data set with known factors, iterated in factor order (what compute_irs requires)."""
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
    got = ev.compute_irs(loader, diff_quantile=0.9, factor_bins=None)
    assert model.training
    model.eval()
    with torch.no_grad():
        mean, _ = model.encoder(images.to(DEV))
    model.train()
    table = mean.cpu().numpy()
    assert_irs(got, table, lat, None, 0.9, None, "encoder means")
    assert got["IRS_matrix"].shape == (int(got["active"].sum()), 3) and 0.0 <= got["IRS"] <= 1.0
    cpu0, dev0 = torch.get_rng_state(), torch.cuda.get_rng_state()
    part, same, other = (ev.compute_irs(loader, n_samples=40, seed=s) for s in (1, 1, 2))
    assert torch.equal(torch.get_rng_state(), cpu0) and torch.equal(torch.cuda.get_rng_state(), dev0)
    assert part["n_samples"] == 40 and part["factor_bins"] == 20 and all(np.array_equal(part[k], same[k]) for k in part)
    assert part["IRS"] != other["IRS"]
    # Evaluator.__call__: with its defaults exactly the file it wrote before; the new one only on request
    ev(loader)
    assert sorted(os.listdir(tmp_path)) == ["test_losses.log"]
    assert ev(loader, is_losses=False, is_irs=True) == (None, None)
    assert sorted(os.listdir(tmp_path)) == ["irs.log", "test_losses.log"]
    logged = json.load(open(tmp_path / "irs.log"))
    assert set(logged) == KEYS and logged["n_samples"] == N and logged["factor_bins"] == 20 and logged["diff_quantile"] == 0.99
    full = ev.compute_irs(loader)
    assert logged["IRS"] == full["IRS"] and logged["IRS_matrix"] == full["IRS_matrix"].tolist() and logged["n_groups"] == [3, 4, 5]
    assert model.training

    class _NoFactors:
        dataset = [0, 1, 2, 3]
    with pytest.raises(ValueError, match="known true factors"):
        ev.compute_irs(_NoFactors())
