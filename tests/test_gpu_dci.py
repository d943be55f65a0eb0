"""GPU: the DCI scores -- the kernels of csrc/boosted_trees.hip (libdvae_dci_hip.so) through the C-ABI, and dci_from_table /
Evaluator.compute_dci on top of them, against the fp64 numpy restatement tests/dci_ref.py.

A fitted model is VERIFIED, not compared (dci_ref.verify): every node of every dumped tree is recomputed in fp64 from the
library's own node membership -- n, sum r and sum r^2 to the accumulation bound 8 S 2^-53 sum |r|, the chosen (feature, threshold)
a legal candidate of a gain >= (1 - 1e-10) x the best gain of that node, the children as the threshold says, leaf values, the
prior and every entry of the raw scores within 1e-12 relative -- which holds whatever happens among splits of equal gain.  On the
cases whose best-vs-second-best gap is >= 1e-9 on 98 % of the nodes (dci_ref.CAP_CASES; test_dci_host.py computes that share from
the restatement alone) the library's choice may differ from the restatement's own first choice on 2 % of the split nodes at the
most; they include both sides of the launcher's switch, a size above 64 KB of LDS and DVAE_DCI_MAX_ROWS.
Measured on the MI355X over all cases below: largest sum error / bound 0.0045, largest relative value error 9.3e-16, other
choices on the cap cases 0 of 94, 0 of 29, 0 of 5, 1 of 340, 0 of 42, 0 of 4, 0 of 17, 0 of 21, 0 of 21.
"""
import json
import logging
import os

import numpy as np
import pytest
import torch

import dci_ref as R
from gpu_util import DEV, stream
from guard_util import Guarded, run_contract
from disvae_amd import _dcilib, Evaluator, dci_from_table
from disvae_amd.models.losses import get_loss_f
from disvae_amd.models.vae import init_specific_model

pytestmark = pytest.mark.gpu
LR = 0.1


def _ptr(t):
    return None if t is None else t.data_ptr()


def _order(X):
    """int32 [D, S]: the stable ascending order of every column"""
    return np.stack([np.argsort(X[:, d], kind="stable") for d in range(X.shape[1])]).astype(np.int32)


def device_fit(table, rows, labels, C, n_stages, raw=None):
    """dvae_dci_fit on table[rows] (rows None: the whole table) -> numpy outputs.  raw: continue from it."""
    X = table if rows is None else table[rows]
    N, D = table.shape
    S, T = X.shape[0], R.trees(C)
    t = {"table": torch.from_numpy(table).to(DEV), "order": torch.from_numpy(_order(X)).to(DEV),
         "rows": None if rows is None else torch.from_numpy(np.asarray(rows, np.int64)).to(DEV),
         "labels": torch.from_numpy(np.asarray(labels, np.int32)).to(DEV),
         "raw": torch.empty(S, T, dtype=torch.float64, device=DEV) if raw is None else torch.from_numpy(raw).to(DEV),
         "prior": torch.empty(T, dtype=torch.float64, device=DEV),
         "ws": torch.empty(_dcilib.lib().dvae_dci_fit_ws_floats(N, D, S, C, n_stages), dtype=torch.float32, device=DEV),
         "importance": torch.empty(D, dtype=torch.float64, device=DEV), "n_split": torch.empty(1, dtype=torch.int32, device=DEV),
         "feature": torch.empty(n_stages, T, R.NODES, dtype=torch.int32, device=DEV),
         "stats": torch.empty(n_stages, T, R.NODES, R.STATS, dtype=torch.float64, device=DEV)}
    assert t["ws"].numel() > 0
    _dcilib.call("dvae_dci_fit", _ptr(t["table"]), _ptr(t["rows"]), _ptr(t["order"]), _ptr(t["labels"]), N, D, S, C, n_stages, LR,
                 1 if raw is None else 0, _ptr(t["raw"]), _ptr(t["prior"]), _ptr(t["ws"]), _ptr(t["importance"]), _ptr(t["n_split"]), _ptr(t["feature"]),
                 _ptr(t["stats"]), stream())
    torch.cuda.synchronize()
    return {k: t[k].cpu().numpy() for k in ("raw", "prior", "importance", "n_split", "feature", "stats")}


def verified(X, labels, C, got, raw_before=None):
    """The prior the library reports within 1e-12 relative of the restatement's, entry by entry; the replay starts from the
    library's own prior (or from raw_before), so that every entry of `raw` is held to 1e-12 relative of it."""
    want = R.prior(np.asarray(labels, np.int64), C)
    assert (np.abs(got["prior"] - want) <= 1e-12 * np.abs(want)).all(), (got["prior"], want)
    if raw_before is None:
        raw_before = np.tile(got["prior"], (len(X), 1))
    out = R.verify(X, labels, C, got["feature"], got["stats"], got["raw"], LR, raw_before)
    assert out["worst_value"] <= 1e-12
    total, n_split = R.importance_of_dump(got["feature"], got["stats"], X.shape[1])
    assert int(got["n_split"][0]) == n_split
    assert np.abs(got["importance"] - total).max() <= 1e-12 * max(np.abs(total).max(), 1e-300)
    print("split nodes %d, other choice than the restatement's %d, worst sum error / bound %.3g, worst value error %.3g"
          % (out["nodes"], out["other_choice"], out["worst_sum"], out["worst_value"]))
    return out


# ---- 1. the fit, verified -------------------------------------------------------------------------------------------------------
def test_narrowest_case_one_stage():
    X, labels, C, n_stages = R.case("narrowest")
    assert (X.shape, C, n_stages) == ((96, 4), 3, 1)
    got = device_fit(X, None, labels, C, n_stages)
    out = verified(X, labels, C, got)
    assert out["nodes"] >= 3 and (got["feature"][0, :, 0] >= 0).all()


@pytest.mark.parametrize("name", [n for n in R.CASES if n != "narrowest"])
def test_fit_is_verified_node_by_node(name):
    X, labels, C, n_stages = R.case(name)
    got = device_fit(X, None, labels, C, n_stages)
    out = verified(X, labels, C, got)
    assert out["nodes"] >= n_stages
    if name in R.CAP_CASES:
        assert out["other_choice"] <= 0.02 * out["nodes"], out
    again = device_fit(X, None, labels, C, n_stages)                     # the same bits on a second run
    assert all(again[k].tobytes() == got[k].tobytes() for k in got)
    if name == "pure":                                                   # a leaf above depth 3 whose sibling goes on
        f = got["feature"].reshape(-1, R.NODES)
        n = got["stats"].reshape(-1, R.NODES, R.STATS)[:, :, 2]
        assert any((f[i, a] < 0 and n[i, a] > 0 and f[i, b] >= 0) for i in range(len(f)) for a, b in ((1, 2), (2, 1)))
    if name in ("basic", "two_class"):                                   # the constant column splits no node
        assert (got["feature"] != 2).all() and got["importance"][2] == 0.0


def test_one_class_present_fits_no_tree():
    X, _labels, _C, _n = R.case("basic")
    labels = np.zeros(len(X), np.int64)
    got = device_fit(X, None, labels, 1, 3)
    assert (got["feature"] == -1).all() and int(got["n_split"][0]) == 0 and not got["importance"].any()
    assert not got["raw"].any() and (got["stats"][:, :, 0, 2] == len(X)).all() and not got["stats"][:, :, 1:].any()
    verified(X, labels, 1, got)


def test_rows_with_repeats():
    table, _l, C, _n = R.case("five_class")
    rng = np.random.default_rng(7)
    rows = rng.integers(0, 150, 96)                                      # many rows drawn twice or more
    assert len(np.unique(rows)) < 80
    labels = rng.integers(0, 3, 96)
    got = device_fit(table, rows, labels, 3, 3)
    verified(table[rows], labels, 3, got)


def test_stages_continue_through_raw():
    X, labels, C, _n = R.case("basic")
    whole = device_fit(X, None, labels, C, 5)
    first = device_fit(X, None, labels, C, 2)
    second = device_fit(X, None, labels, C, 3, raw=first["raw"])
    assert second["raw"].tobytes() == whole["raw"].tobytes()
    for k in ("feature", "stats"):
        assert np.concatenate([first[k], second[k]]).tobytes() == whole[k].tobytes()
    assert int(first["n_split"][0]) + int(second["n_split"][0]) == int(whole["n_split"][0])
    assert np.abs(first["importance"] + second["importance"] - whole["importance"]).max() <= 1e-12 * whole["importance"].max()
    verified(X, labels, C, second, raw_before=first["raw"])


# ---- 2. predict -------------------------------------------------------------------------------------------------------------------
def device_predict(table, rows, C, got, prior):
    S = table.shape[0] if rows is None else len(rows)
    t_table, t_rows = torch.from_numpy(table).to(DEV), None if rows is None else torch.from_numpy(np.asarray(rows, np.int64)).to(DEV)
    feature, stats = torch.from_numpy(got["feature"]).to(DEV), torch.from_numpy(got["stats"]).to(DEV)
    raw = torch.from_numpy(np.tile(prior, (S, 1))).to(DEV)
    _dcilib.call("dvae_dci_predict", _ptr(t_table), _ptr(t_rows), table.shape[0], table.shape[1], S, C, got["feature"].shape[0], LR,
                 _ptr(feature), _ptr(stats), _ptr(raw), stream())
    torch.cuda.synchronize()
    return raw.cpu().numpy()


@pytest.mark.parametrize("name", ["basic", "two_class", "five_class"])
def test_predict_is_the_restatements_evaluation_of_the_dump(name):
    X, labels, C, n_stages = R.case(name)
    got = device_fit(X, None, labels, C, n_stages)
    prior = got["prior"]
    assert device_predict(X, None, C, got, prior).tobytes() == got["raw"].tobytes()          # on the rows of the fit: its bits
    held_out, _labels = R.table(131, X.shape[1], C, 99, "mixed")
    rows = np.random.default_rng(3).integers(0, 131, 77)
    for r in (None, rows):
        raw = device_predict(held_out, r, C, got, prior)
        want = R.predict(held_out if r is None else held_out[r], got["feature"], got["stats"], np.tile(prior, (len(raw), 1)), LR)
        assert (np.abs(raw - want) <= 1e-12 * np.abs(want)).all()
        assert np.array_equal(R.classes_of(raw, C), R.classes_of(want, C))


# ---- 3. memory contract ---------------------------------------------------------------------------------------------------------
def _dci_call(name):
    def fn(args):
        _dcilib.call(name, *[a.ptr if isinstance(a, Guarded) else a for a in args])
    return fn


@pytest.mark.parametrize("name,with_rows", [("basic", False), ("two_class", True), ("chunk_above", True)])
def test_memory_contract_fit(name, with_rows):
    X, labels, C, n_stages = R.case(name)
    n_stages = min(n_stages, 2)
    rows = np.random.default_rng(5).integers(0, len(X), len(X)) if with_rows else None
    Xs = X if rows is None else X[rows]
    N, D = X.shape
    S, T = len(Xs), R.trees(C)
    nws = _dcilib.lib().dvae_dci_fit_ws_floats(N, D, S, C, n_stages)

    def build(al):
        r = None if rows is None else al.inp("rows", rows.astype(np.int64), align=8)
        return [al.inp("table", X, align=4), r, al.inp("order", _order(Xs), align=4), al.inp("labels", labels.astype(np.int32), align=4),
                N, D, S, C, n_stages, LR, 1, al.out("raw", (S, T), dtype=torch.float64, align=8),
                al.out("prior", (T,), dtype=torch.float64, align=8), al.ws("ws", (nws,), align=8),
                al.out("importance", (D,), dtype=torch.float64, align=8), al.out("n_split", (1,), dtype=torch.int32, align=4),
                al.out("feature", (n_stages, T, R.NODES), dtype=torch.int32, align=4),
                al.out("stats", (n_stages, T, R.NODES, R.STATS), dtype=torch.float64, align=8), stream()]
    runs = run_contract("dvae_dci_fit", build, fn=_dci_call("dvae_dci_fit"))
    plain = {g.name: g.t.cpu().numpy() for g in runs[0].args}
    got = device_fit(X, rows, labels, C, n_stages)
    assert all(plain[k].tobytes() == got[k].tobytes() for k in ("raw", "prior", "importance", "n_split", "feature", "stats"))


def test_memory_contract_predict():
    X, labels, C, n_stages = R.case("basic")
    got = device_fit(X, None, labels, C, n_stages)
    prior = got["prior"]
    rows = np.random.default_rng(6).integers(0, len(X), 70)
    for r in (None, rows):
        S = len(X) if r is None else len(r)

        def build(al):
            rr = None if r is None else al.inp("rows", r.astype(np.int64), align=8)
            return [al.inp("table", X, align=4), rr, len(X), X.shape[1], S, C, n_stages, LR, al.inp("feature", got["feature"], align=4),
                    al.inp("stats", got["stats"], align=8, dtype=torch.float64),
                    al.inout("raw", np.tile(prior, (S, 1)), align=8, dtype=torch.float64), stream()]
        runs = run_contract("dvae_dci_predict", build, fn=_dci_call("dvae_dci_predict"))
        assert runs[0].args[-1].t.cpu().numpy().tobytes() == device_predict(X, r, C, got, prior).tobytes()


# ---- 4. end to end ----------------------------------------------------------------------------------------------------------------
def _ideal_table(rotated):
    """latent d = factor d plus small noise over all 60 combinations of lat_sizes (3, 4, 5)"""
    sizes = (3, 4, 5)
    factors = np.stack(np.meshgrid(*[np.arange(k) for k in sizes], indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float64)
    z = factors + 0.05 * np.random.default_rng(0).standard_normal(factors.shape)
    if rotated:                                                          # 45 degrees in the plane of two informative latents
        c = np.sqrt(0.5)
        z[:, :2] = z[:, :2] @ np.array([[c, -c], [c, c]])
    return torch.from_numpy(z.astype(np.float32)).to(DEV), sizes


def test_dci_from_table_orders_an_ideal_and_a_rotated_representation():
    rows = np.tile(np.arange(60), 5)                                     # every combination four times to fit, once to test
    scores = []
    for rotated in (False, True):
        mean, sizes = _ideal_table(rotated)
        got = dci_from_table(mean, sizes, n_train=240, n_test=60, rows=rows, n_stages=10)
        assert got["importance_matrix"].shape == (3, 3) and np.allclose(got["importance_matrix"].sum(axis=0), 1.0, atol=1e-12)
        assert got["n_train"] == 240 and got["n_test"] == 60 and got["n_stages"] == 10
        print(rotated, {k: v for k, v in got.items() if k != "importance_matrix"})
        scores.append(got)
    ideal, rotated = scores
    assert ideal["disentanglement"] > 0.9 and ideal["completeness"] > 0.9
    assert ideal["informativeness_train"] == 1.0 and ideal["informativeness_test"] == 1.0
    assert rotated["disentanglement"] < ideal["disentanglement"] - 0.1 and rotated["completeness"] < ideal["completeness"] - 0.1
    again = dci_from_table(_ideal_table(True)[0], (3, 4, 5), n_train=40, n_test=20, seed=3, n_stages=2)     # drawn rows: the same bits
    once_more = dci_from_table(_ideal_table(True)[0], (3, 4, 5), n_train=40, n_test=20, seed=3, n_stages=2)
    assert again["importance_matrix"].tobytes() == once_more["importance_matrix"].tobytes()


class _Factors:
    lat_sizes, lat_names = np.array([3, 4, 5]), ("a", "b", "c")

    def __init__(self, images):
        self.images = images

    def __len__(self):
        return self.images.shape[0]


class _Loader:
    def __init__(self, images, bs):
        self.dataset, self.bs = _Factors(images), bs

    def __len__(self):
        return (len(self.dataset) + self.bs - 1) // self.bs

    def __iter__(self):
        for i in range(0, len(self.dataset), self.bs):
            yield self.dataset.images[i:i + self.bs], 0


def test_evaluator_end_to_end(tmp_path):
    img, N, D = (1, 32, 32), 60, 4
    torch.manual_seed(3)
    model = init_specific_model("Burgess", img, D)
    loss_f = get_loss_f("btcvae", device=torch.device(DEV), n_data=N, rec_dist="bernoulli", reg_anneal=0, btcvae_A=1, btcvae_B=6,
                        btcvae_G=1)
    loader = _Loader(torch.rand((N,) + img, generator=torch.Generator().manual_seed(4)), 32)
    ev = Evaluator(model, loss_f, device=torch.device(DEV), logger=logging.getLogger("dci"), save_dir=str(tmp_path), is_progress_bar=False)
    model.train()
    args = dict(n_train=40, n_test=20, n_stages=3)
    got = ev.compute_dci(loader, **args)
    assert model.training
    keys = {"disentanglement", "completeness", "informativeness_train", "informativeness_test", "importance_matrix", "n_train", "n_test",
            "n_stages"}
    assert set(got) == keys and got["importance_matrix"].shape == (D, 3)
    assert 0.0 <= got["disentanglement"] <= 1.0 and 0.0 <= got["completeness"] <= 1.0 and 0.0 <= got["informativeness_test"] <= 1.0
    _none, losses = ev(loader)
    assert sorted(os.listdir(tmp_path)) == ["test_losses.log"]          # with the default nothing new is written
    ev(loader, is_losses=False, is_dci=True, dci_args=args)
    assert sorted(os.listdir(tmp_path)) == ["dci.log", "test_losses.log"]
    logged = json.load(open(tmp_path / "dci.log"))
    assert set(logged) == keys - {"importance_matrix"}
    assert all(logged[k] == got[k] for k in logged)
