"""GPU: the prediction-based scores -- downstream_task_from_table, fairness_from_table, explicitness_from_table and the three
Evaluator.compute_* on top of them -- on the entry points that are there: dvae_dci_fit / dvae_dci_predict (libdvae_dci_hip.so) and
dvae_udr_ranks (libdvae_udr_hip.so).  The kernels have their own tests (test_gpu_dci.py, test_gpu_udr.py); here the scores are held
to dci_from_table bit for bit (the same launches), to the numpy restatement tests/predict_ref.py applied to the device's own
predictions and probabilities, to scikit-learn's hull of eight seeds, and to what an ideal and an entangled table must give.
Tables: predict_ref's fixtures, lat_sizes (3, 4, 5) (N = 60) and (4, 6, 8, 5) (N = 960), D = 6; 10 stages."""
import json
import logging
import os

import numpy as np
import pytest
import torch

import predict_ref as P
from gpu_util import DEV
from disvae_amd import (_dcilib, Evaluator, dci_from_table, downstream_task_from_table, explicitness_from_table,
                        fairness_from_table)
from disvae_amd.models.losses import get_loss_f
from disvae_amd.models.vae import init_specific_model

pytestmark = pytest.mark.gpu
STAGES = 10
N_TEST = {P.SMALL: 20, P.LARGE: 200}
FAIRNESS_KEYS = {"mean_unfairness_matrix", "max_unfairness_matrix", "mean_unfairness", "max_unfairness", "mean_unfairness_per_target",
                 "mean_unfairness_per_sensitive", "n_train", "n_test_per_value", "n_stages"}
EXPLICITNESS_KEYS = {"explicitness_train", "explicitness_test", "explicitness_train_per_factor", "explicitness_test_per_factor",
                     "n_train", "n_test"}


def _dev(table):
    return torch.from_numpy(table).to(DEV)


def _same(a, b):
    """two results: the same keys, the same bits"""
    assert set(a) == set(b)
    return all((np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes()) for k in a)


# ---- 1. downstream task -------------------------------------------------------------------------------------------------------
_DOWNSTREAM = {}


def _downstream(sizes, ns):
    """One call per table, shared by the tests below: (result, the injected rows per size)"""
    if sizes not in _DOWNSTREAM:
        table = _dev(P.entangled_table(sizes))
        rows = [P.drawn_rows(len(table), n + N_TEST[sizes], n) for n in ns]
        got = downstream_task_from_table(table, sizes, n_train=ns, n_test=N_TEST[sizes], rows=rows, n_stages=STAGES)
        _DOWNSTREAM[sizes] = (got, rows, table)
    return _DOWNSTREAM[sizes]


@pytest.mark.parametrize("sizes, ns", [(P.SMALL, (10, 30)), (P.LARGE, (100, 400))], ids=["N60", "N960"])
def test_downstream_is_dci_from_table_bit_for_bit(sizes, ns):
    got, rows, table = _downstream(sizes, ns)
    assert set(got) == P.downstream_keys(ns, len(sizes)) | {"n_train", "n_test", "n_stages"}
    assert (got["n_train"], got["n_test"], got["n_stages"]) == (list(ns), N_TEST[sizes], STAGES)
    for n, rows_n in zip(ns, rows):
        dci = dci_from_table(table, sizes, n_train=n, n_test=N_TEST[sizes], rows=rows_n, n_stages=STAGES)
        print(n, got["%d:mean_train_accuracy" % n], got["%d:mean_test_accuracy" % n])
        assert got["%d:mean_test_accuracy" % n] == dci["informativeness_test"]           # the same launches: the same bits
        assert got["%d:mean_train_accuracy" % n] == dci["informativeness_train"]
    K = len(sizes)
    acc = {name: np.array([[got["%d:%s_accuracy_factor_%d" % (n, name, k)] for k in range(K)] for n in ns]) for name in ("train", "test")}
    want = P.downstream_aggregates(list(ns), acc["train"], acc["test"])
    assert all(abs(got[key] - value) <= 1e-15 for key, value in want.items())
    assert got["%d:efficiency" % ns[0]] == got["%d:mean_test_accuracy" % ns[0]] / got["%d:mean_test_accuracy" % ns[1]]
    assert all(type(v) is float for k, v in got.items() if ":" in k)


def test_downstream_accuracies_within_the_hull_of_eight_sklearn_seeds():
    """The rule of tests/dci_ref.py (test_dci_host.py): every factor's train and test accuracy on the N = 960 table, 100 and 400
    training rows, inside the min-max hull of GradientBoostingClassifier(n_estimators=10, random_state = 0 .. 7) widened by 25 %
    of its width and never by less than 1e-12.  The restatement is held to the same hull on the CPU
    (test_prediction_scores_host.py)."""
    from sklearn import ensemble                                         # the yardstick: no skip without it
    sizes, ns = P.LARGE, (100, 400)
    got, rows, _table = _downstream(sizes, ns)
    table = P.entangled_table(sizes)
    for n, rows_n in zip(ns, rows):
        train, test = rows_n[:n], rows_n[n:]
        for k, stride in enumerate(P.strides(sizes)):
            ours = np.array([got["%d:train_accuracy_factor_%d" % (n, k)], got["%d:test_accuracy_factor_%d" % (n, k)]])
            v_train, v_test = (train // stride) % sizes[k], (test // stride) % sizes[k]
            seeds = []
            for seed in range(8):
                model = ensemble.GradientBoostingClassifier(n_estimators=STAGES, random_state=seed).fit(table[train], v_train)
                seeds.append((model.score(table[train], v_train), model.score(table[test], v_test)))
            lo, hi = np.min(seeds, axis=0), np.max(seeds, axis=0)
            widen = np.maximum(0.25 * (hi - lo), 1e-12)
            print("n = %d, factor %d: %s, hull %s .. %s" % (n, k, ours, lo, hi))
            assert ((ours >= lo - widen) & (ours <= hi + widen)).all(), (n, k, ours, lo, hi)


# ---- 2. the ideal table -------------------------------------------------------------------------------------------------------
def test_ideal_table_downstream_and_fairness():
    """Latent k is factor k plus noise below a quarter of a step.  Test accuracy is 1.0 from the size at which every value of every
    factor is among the training rows (the 10-row draw misses one: test_prediction_scores_host.py states both from the
    restatement); with every row in the fit every prediction is the row's own value, whatever is intervened on: unfairness 0."""
    sizes = P.SMALL
    table = _dev(P.ideal_table(sizes))
    ns = (10, 40)
    rows = [P.drawn_rows(60, n + 20, n) for n in ns]
    got = downstream_task_from_table(table, sizes, n_train=ns, n_test=20, rows=rows, n_stages=STAGES)
    complete = [all(len(np.unique((r[:n] // s) % size)) == size for s, size in zip(P.strides(sizes), sizes)) for n, r in zip(ns, rows)]
    assert complete == [False, True]
    print({k: v for k, v in got.items() if "mean" in k or "efficiency" in k})
    assert got["40:min_test_accuracy"] == 1.0 and got["40:mean_test_accuracy"] == 1.0 and got["40:min_train_accuracy"] == 1.0
    assert got["10:min_train_accuracy"] == 1.0 and got["10:min_test_accuracy"] < 1.0     # a value never seen counts as an error
    assert got["10:efficiency"] == got["10:mean_test_accuracy"] < 1.0
    fair = fairness_from_table(table, sizes, n_train=60, n_test_per_value=7, seed=2, n_stages=STAGES, rows=np.arange(60))
    assert set(fair) == FAIRNESS_KEYS
    assert not fair["mean_unfairness_matrix"].any() and not fair["max_unfairness_matrix"].any()       # exactly 0 everywhere
    assert fair["mean_unfairness"] == 0.0 and fair["max_unfairness"] == 0.0
    assert (fair["n_train"], fair["n_test_per_value"], fair["n_stages"]) == (60, 7, STAGES)


def test_ideal_table_explicitness_is_one():
    """On the ideal N = 960 table (600 rows to fit, 360 to test; on the CPU, test_prediction_scores_host.py's measurement) the
    logistic regression ranks every class's rows above all others: every AUC is exactly 1."""
    sizes = P.LARGE
    got = explicitness_from_table(_dev(P.ideal_table(sizes)), sizes, n_train=600, n_test=360, rows=P.drawn_rows(960, 960, 1))
    assert set(got) == EXPLICITNESS_KEYS and (got["n_train"], got["n_test"]) == (600, 360)
    print(got)
    assert got["explicitness_train"] == 1.0 and got["explicitness_test"] == 1.0
    assert (got["explicitness_train_per_factor"] == 1.0).all() and (got["explicitness_test_per_factor"] == 1.0).all()


# ---- 3. the entangled table ---------------------------------------------------------------------------------------------------
def _check_fairness_against_the_restatement(got, details, sizes, base_rows):
    """every matrix entry is predict_ref's unfairness of the device's own predicted values, and one row has one prediction"""
    K = len(sizes)
    for i in range(K):
        seen = {}
        for j in range(K):
            if i == j:
                assert got["mean_unfairness_matrix"][i, i] == 0.0 and got["max_unfairness_matrix"][i, i] == 0.0
                continue
            predicted = details["predicted"][i, j].numpy()
            assert predicted.shape == (sizes[j], base_rows.shape[2])
            want = P.unfairness(P.counts_of(predicted, details["classes"][i].numpy()))
            assert (got["mean_unfairness_matrix"][i, j], got["max_unfairness_matrix"][i, j]) == want, (i, j)
            for r, v in zip(P.intervened(base_rows[i, j], sizes, j).reshape(-1), predicted.reshape(-1)):
                assert seen.setdefault(int(r), int(v)) == int(v), (i, j, r)
    want = P.fairness_aggregates(got["mean_unfairness_matrix"], got["max_unfairness_matrix"])
    assert all(np.allclose(got[key], value, rtol=0, atol=1e-15) for key, value in want.items())


def test_entangled_table_fairness():
    """Latent 0 is v_0 + 3 v_1: what is predicted for factor 0 moves with factor 1."""
    sizes = P.SMALL
    table = _dev(P.entangled_table(sizes))
    base_rows = np.random.default_rng(5).integers(0, 60, (3, 3, 6))
    got, details = fairness_from_table(table, sizes, n_train=40, n_test_per_value=6, n_stages=STAGES, rows=P.drawn_rows(60, 40, 3),
                                       base_rows=base_rows, return_details=True)
    assert set(got) == FAIRNESS_KEYS
    print(got["mean_unfairness_matrix"], got["max_unfairness_matrix"])
    assert got["mean_unfairness_matrix"][0, 1] > 0
    assert (got["max_unfairness_matrix"] >= got["mean_unfairness_matrix"]).all() and got["max_unfairness_matrix"].max() <= 1.0
    _check_fairness_against_the_restatement(got, details, sizes, base_rows)


_EXPLICITNESS = {}


def _entangled_explicitness():
    """One call, shared: the N = 60 entangled table; the 12 test rows hold no row with factor 2 = 4 (a class without positives
    there) and the 40 training rows none with factor 1 = 3 (test rows of a value never seen)."""
    if not _EXPLICITNESS:
        sizes = P.SMALL
        factors = P.factor_table(sizes)
        order = np.random.default_rng(9).permutation(60)
        train = [r for r in order if factors[r, 1] != 3][:40]
        rest = [r for r in order if r not in train and factors[r, 2] != 4]
        test = sorted(rest, key=lambda r: factors[r, 1] == 3)[:12]       # the few left of the values seen, then rows of the unseen one
        assert len(train) == 40 and len(test) == 12 and (factors[train, 2] == 4).any()
        assert (factors[test, 1] == 3).any() and (factors[test, 1] != 3).any()
        states = torch.get_rng_state(), torch.cuda.get_rng_state()
        got, details = explicitness_from_table(_dev(P.entangled_table(sizes)), sizes, n_train=40, n_test=12,
                                               rows=np.array(train + test), return_details=True)
        unchanged = torch.equal(states[0], torch.get_rng_state()) and torch.equal(states[1], torch.cuda.get_rng_state())
        _EXPLICITNESS.update(got=got, details=details, unchanged=unchanged)
    return _EXPLICITNESS


def test_entangled_table_explicitness_is_the_restatement_on_the_devices_probabilities():
    shared = _entangled_explicitness()
    got, details = shared["got"], shared["details"]
    assert set(got) == EXPLICITNESS_KEYS and shared["unchanged"]
    print(got)
    for k, d in enumerate(details):
        for name in ("train", "test"):
            prob, labels = d["probabilities_" + name].numpy(), d["labels_" + name].numpy()
            assert prob.dtype == np.float32 and prob.shape == (len(labels), len(d["classes"]))
            auc, macro = P.ovr_auc(prob, labels)
            assert d["auc_" + name].tobytes() == auc.tobytes(), (k, name)              # byte for byte
            assert np.float64(got["explicitness_%s_per_factor" % name][k]).tobytes() == np.float64(macro).tobytes()
    for name in ("train", "test"):
        per_factor = got["explicitness_%s_per_factor" % name]
        assert got["explicitness_" + name] == float(np.mean(per_factor[~np.isnan(per_factor)]))
    # latent 0 orders factor 1; factor 2 is in no latent
    assert got["explicitness_train_per_factor"][1] > got["explicitness_train_per_factor"][2]


def test_explicitness_edge_cases():
    """A class without positives among the test rows is left out of its factor's mean; a test row whose value was never seen in
    training is a negative of every class."""
    details = _entangled_explicitness()["details"]
    assert details[2]["classes"].tolist() == [0, 1, 2, 3, 4] and not (details[2]["labels_test"] == 4).any()
    assert np.isnan(details[2]["auc_test"][4]) and not np.isnan(details[2]["auc_train"]).any()
    assert details[1]["classes"].tolist() == [0, 1, 2] and (details[1]["labels_test"] == -1).any()
    for d in details:                                                    # an AUC is missing exactly where a class has no positives
        labels = d["labels_test"].numpy()
        missing = np.array([(labels == v).sum() in (0, len(labels)) for v in range(len(d["classes"]))])
        assert np.array_equal(np.isnan(d["auc_test"]), missing)


# ---- 4. edge cases of the boosted scores ----------------------------------------------------------------------------------------
def test_a_training_draw_that_misses_a_value_and_one_with_one_value_present():
    sizes = P.SMALL
    factors = P.factor_table(sizes)
    table = _dev(P.entangled_table(sizes))
    base_rows = np.random.default_rng(6).integers(0, 60, (3, 3, 5))
    # (a) no training row has factor 2 = 4: four classes; the test rows that have it are errors
    train = np.flatnonzero(factors[:, 2] != 4)
    test = np.flatnonzero(factors[:, 2] == 4)
    got = downstream_task_from_table(table, sizes, n_train=(48,), n_test=12, rows=[np.concatenate([train, test])], n_stages=STAGES)
    assert got["48:test_accuracy_factor_2"] == 0.0
    fair, details = fairness_from_table(table, sizes, n_train=48, n_test_per_value=5, n_stages=STAGES, rows=train, base_rows=base_rows,
                                        return_details=True)
    assert details["classes"][2].tolist() == [0, 1, 2, 3] and int(details["predicted"][2, 0].max()) <= 3
    _check_fairness_against_the_restatement(fair, details, sizes, base_rows)
    # (b) every training row has factor 0 = 1: no tree is fitted, 1 is predicted everywhere
    train = np.flatnonzero(factors[:, 0] == 1)
    test = np.array([0, 20, 21, 40, 59, 22])                                              # three of six have factor 0 = 1
    got = downstream_task_from_table(table, sizes, n_train=(20,), n_test=6, rows=[np.concatenate([train, test])], n_stages=STAGES)
    assert got["20:train_accuracy_factor_0"] == 1.0 and got["20:test_accuracy_factor_0"] == 3 / 6
    fair, details = fairness_from_table(table, sizes, n_train=20, n_test_per_value=5, n_stages=STAGES, rows=train, base_rows=base_rows,
                                        return_details=True)
    assert details["classes"][0].tolist() == [1] and (details["predicted"][0, 1] == 1).all() and (details["predicted"][0, 2] == 1).all()
    assert not fair["mean_unfairness_matrix"][0].any() and not fair["max_unfairness_matrix"][0].any()
    _check_fairness_against_the_restatement(fair, details, sizes, base_rows)
    expl = explicitness_from_table(table, sizes, n_train=20, n_test=6, rows=np.concatenate([train, test]))
    # the one class has no negatives among the training rows: no AUC; among the test rows the three rows of values never seen
    # are its negatives and every probability is 1: all ties, 0.5
    assert np.isnan(expl["explicitness_train_per_factor"][0]) and expl["explicitness_test_per_factor"][0] == 0.5
    assert expl["explicitness_train"] == float(np.mean(expl["explicitness_train_per_factor"][1:]))


def test_predictions_above_the_row_limit_of_one_call():
    """A sensitive factor of 128 values with 100 base rows: 12 800 intervened rows, more than DVAE_DCI_MAX_ROWS, go through two
    dvae_dci_predict calls.  Latent 0 is factor 1 plus small noise and every row is in the fit, so every prediction of factor 1 is
    the base row's own value on both sides of the split."""
    sizes, per_value = (128, 3), 100
    assert sizes[0] * per_value > _dcilib.MAX_ROWS
    rng = np.random.default_rng(7)
    factors = P.factor_table(sizes)
    z = np.stack([factors[:, 1] + rng.uniform(-0.2, 0.2, 384), factors[:, 0] / 16.0 + rng.uniform(-0.01, 0.01, 384)], axis=1)
    base_rows = rng.integers(0, 384, (2, 2, per_value))
    got, details = fairness_from_table(_dev(z.astype(np.float32)), sizes, n_train=384, n_test_per_value=per_value, n_stages=3,
                                       rows=np.arange(384), base_rows=base_rows, return_details=True)
    predicted = details["predicted"][1, 0].numpy()
    assert predicted.shape == (128, per_value)
    assert (predicted == factors[base_rows[1, 0], 1][None, :]).all()                      # also past row 10 240 of the 12 800
    assert got["mean_unfairness_matrix"][1, 0] == 0.0 and got["max_unfairness_matrix"][1, 0] == 0.0
    _check_fairness_against_the_restatement(got, details, sizes, base_rows)


# ---- 5. determinism -------------------------------------------------------------------------------------------------------------
def test_the_same_seed_gives_the_same_bits_and_the_global_generators_stay():
    sizes = P.SMALL
    table = _dev(P.entangled_table(sizes))
    torch.manual_seed(11)
    torch.cuda.manual_seed(12)
    states = torch.get_rng_state(), torch.cuda.get_rng_state()
    down = [downstream_task_from_table(table, sizes, n_train=(10, 30), n_test=20, seed=s, n_stages=STAGES) for s in (4, 4, 5)]
    fair = [fairness_from_table(table, sizes, n_train=40, n_test_per_value=6, seed=s, n_stages=STAGES, return_details=True) for s in (4, 4, 5)]
    assert torch.equal(states[0], torch.get_rng_state()) and torch.equal(states[1], torch.cuda.get_rng_state())
    assert _same(down[0], down[1]) and not _same(down[0], down[2])
    assert _same(fair[0][0], fair[1][0]) and not _same(fair[0][0], fair[2][0])
    assert all(torch.equal(fair[0][1]["predicted"][ij], fair[1][1]["predicted"][ij]) for ij in fair[0][1]["predicted"])
    # the first draw of the downstream task is dci_from_table's draw of that seed
    dci = dci_from_table(table, sizes, n_train=10, n_test=20, seed=4, n_stages=STAGES)
    assert down[0]["10:mean_test_accuracy"] == dci["informativeness_test"]


# ---- 6. Evaluator ---------------------------------------------------------------------------------------------------------------
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
    ev = Evaluator(model, loss_f, device=torch.device(DEV), logger=logging.getLogger("prediction"), save_dir=str(tmp_path),
                   is_progress_bar=False)
    model.train()
    args = {"downstream": dict(n_train=(10, 30), n_test=20, n_stages=3), "fairness": dict(n_train=40, n_test_per_value=4, n_stages=3),
            "explicitness": dict(n_train=40, n_test=20)}
    got = {"downstream_task": ev.compute_downstream_task(loader, **args["downstream"]), "fairness": ev.compute_fairness(loader, **args["fairness"]),
           "explicitness": ev.compute_explicitness(loader, **args["explicitness"])}
    assert model.training
    assert set(got["downstream_task"]) == P.downstream_keys((10, 30), 3) | {"n_train", "n_test", "n_stages"}
    assert set(got["fairness"]) == FAIRNESS_KEYS and got["fairness"]["mean_unfairness_matrix"].shape == (3, 3)
    assert set(got["explicitness"]) == EXPLICITNESS_KEYS and got["explicitness"]["explicitness_test_per_factor"].shape == (3,)
    assert 0.0 <= got["downstream_task"]["30:mean_test_accuracy"] <= 1.0 and 0.0 <= got["fairness"]["mean_unfairness"] <= 1.0
    assert 0.0 <= got["explicitness"]["explicitness_test"] <= 1.0
    ev(loader)
    assert sorted(os.listdir(tmp_path)) == ["test_losses.log"]          # with the default flags nothing new is written
    ev(loader, is_losses=False, is_downstream=True, is_fairness=True, is_explicitness=True, downstream_args=args["downstream"],
       fairness_args=args["fairness"], explicitness_args=args["explicitness"])
    assert sorted(os.listdir(tmp_path)) == ["downstream_task.log", "explicitness.log", "fairness.log", "test_losses.log"]
    for name, result in got.items():
        logged = json.load(open(tmp_path / (name + ".log")))
        assert set(logged) == set(result)
        for key, value in result.items():
            assert logged[key] == (value.tolist() if isinstance(value, np.ndarray) else value), (name, key)
