"""CPU: the host side of the prediction-based scores -- downstream task, fairness, explicitness (disvae_amd.evaluate) -- against the
numpy restatement tests/predict_ref.py and the installed scikit-learn: the AUC from rank sums, the unfairness of a count matrix,
the row arithmetic of an intervention, the aggregates and the exact key names, the argument errors raised before any device work,
the logistic regression behind explicitness, and the preconditions of the GPU tests from the boosted-tree restatement
(tests/dci_ref.py) alone.

Explicitness against scikit-learn 1.7.2 (LogisticRegression(C=1.0, max_iter=10000, tol=1e-10) + roc_auc_score per class), measured
on the CPU on the ideal and the entangled table of both fixtures (predict_ref; rows drawn_rows(N, 40 + 20 | 600 + 360, seed 1)),
every factor, train and test rows: the largest |difference| of a factor's AUC is 6.78e-6 (the entangled N = 960 table, factor 3,
train rows: an AUC near 0.57, where two all-but-tied pairs of scores order differently), 0 in 27 of the 28 comparisons; the
coefficients differ by 1.6e-7 to 3.3e-5.  An AUC moves in steps of 1 / (n+ n-), so the bound is 4 x the largest measured value,
2.8e-5 (under the cap of 1e-3).  The test runs the two entangled tables (the ideal ones took part in the measurement only).
"""
import json

import numpy as np
import pytest
import torch

import dci_ref as R
import predict_ref as P
import disvae_amd
from disvae_amd import _dcilib, _lib, _udrlib
from disvae_amd import evaluate as E

EXPLICITNESS_MEASURED = 6.78e-6
EXPLICITNESS_BOUND = 4 * EXPLICITNESS_MEASURED
assert EXPLICITNESS_BOUND <= 1e-3


# ---- 1. AUC -------------------------------------------------------------------------------------------------------------------
def _score_tables():
    """name -> (scores fp32 [S, C], labels [S]): heavy ties, a constant column, perfectly separated classes, plain noise"""
    rng = np.random.default_rng(0)
    S, C = 300, 4
    labels = rng.integers(0, C, S)
    noise = rng.standard_normal((S, C))
    out = {"noise": (noise + 0.7 * np.eye(C)[labels], labels),
           "heavy ties": (np.round(noise + 0.7 * np.eye(C)[labels]), labels),                  # a handful of distinct values
           "two values": ((noise + np.eye(C)[labels] > 0.5).astype(np.float64), labels),
           "separated": (np.eye(C)[labels] * 5.0 + rng.uniform(0, 1, (S, C)), labels)}
    constant = noise.copy()
    constant[:, 2] = 0.25
    out["constant column"] = (constant, labels)
    near = np.float64(np.float32(0.3)) + 1e-9 * rng.standard_normal((S, C))                     # equal once rounded to fp32
    out["ties by rounding"] = (near, labels)
    return {k: (v.astype(np.float32), lab) for k, (v, lab) in out.items()}


@pytest.mark.parametrize("name", list(_score_tables()))
def test_auc_is_sklearns(name):
    """The restatement's and evaluate's AUC (ranks written out / rank sums) against roc_auc_score on the fp32 scores, binary per
    class and macro one-vs-rest.  roc_auc_score integrates the ROC curve by trapezoids, up to S terms of at most 1: S 2^-52."""
    from sklearn.metrics import roc_auc_score                            # the yardstick: no skip without it
    scores, labels = _score_tables()[name]
    S, C = scores.shape
    tol = S * 2.0 ** -52
    want = np.array([roc_auc_score(labels == v, scores[:, v]) for v in range(C)])
    auc, macro = P.ovr_auc(scores, labels)
    assert np.abs(auc - want).max() <= tol and abs(macro - want.mean()) <= tol
    ranks = np.stack([P.average_ranks(scores[:, v]) for v in range(C)], axis=1)
    rank_sum = np.array([ranks[labels == v, v].sum() for v in range(C)])
    got, got_macro = E.auc_from_rank_sums(rank_sum, np.bincount(labels, minlength=C), S)
    assert got.tobytes() == auc.tobytes() and got_macro == macro         # the two restatements: the same bits
    if name == "constant column":
        assert auc[2] == 0.5
    if name == "separated":
        assert (auc == 1.0).all() and macro == 1.0
    if name == "ties by rounding":
        assert (auc == 0.5).all()
    if name == "noise":                                                  # the library form of macro one-vs-rest on probabilities
        prob = torch.softmax(torch.from_numpy(scores), dim=1).numpy()
        prob = prob / prob.sum(axis=1, keepdims=True, dtype=np.float64)  # roc_auc_score wants rows that sum to 1
        assert abs(P.ovr_auc(prob, labels)[1] - roc_auc_score(labels, prob, multi_class="ovr", average="macro")) <= tol


def test_average_ranks_are_scipys():
    from scipy import stats
    rng = np.random.default_rng(1)
    for x in (rng.integers(0, 5, 200).astype(np.float32), rng.standard_normal(100).astype(np.float32), np.zeros(7, np.float32)):
        assert P.average_ranks(x).tobytes() == stats.rankdata(x, method="average").astype(np.float64).tobytes()


def test_auc_leaves_out_a_class_without_positives_or_negatives():
    scores = np.random.default_rng(2).random((20, 3)).astype(np.float32)
    labels = np.array([0] * 12 + [1] * 8)                                # class 2 has no positives
    auc, macro = P.ovr_auc(scores, labels)
    assert np.isnan(auc[2]) and not np.isnan(auc[:2]).any() and macro == float(np.mean(auc[:2]))
    labels = np.array([-1] * 5 + [1] * 15)                               # rows of a value never seen: negatives of every class
    auc, macro = P.ovr_auc(scores, labels)
    assert np.isnan(auc[0]) and np.isnan(auc[2]) and macro == auc[1]
    auc, macro = P.ovr_auc(scores[:, :1], np.zeros(20, np.int64))        # one class, no negatives: nothing to average
    assert np.isnan(auc).all() and np.isnan(macro)
    got, got_macro = E.auc_from_rank_sums(np.array([210.0]), np.array([20]), 20)
    assert np.isnan(got).all() and np.isnan(got_macro)
    got = E.explicitness_from_aucs([np.nan, 0.75], [np.nan, np.nan])
    assert got["explicitness_train"] == 0.75 and np.isnan(got["explicitness_test"])


# ---- 2. unfairness ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unfairness", [P.unfairness, E.unfairness_from_counts], ids=["reference", "evaluate"])
def test_unfairness_of_hand_made_counts(unfairness):
    assert unfairness([[3, 3, 3], [7, 7, 7], [0, 0, 0]]) == (0.0, 0.0)   # identical columns: exactly 0
    assert unfairness([[10, 0], [0, 10]]) == (0.5, 0.5)                  # two disjoint columns of equal weight
    assert unfairness([[4, 0], [0, 4], [0, 0]]) == (0.5, 0.5)
    # unequal weights: columns (30, 0) and (0, 10); overall (0.75, 0.25); tv = 0.25 and 0.75; mean (30 0.25 + 10 0.75) / 40
    mean, largest = unfairness([[30, 0], [0, 10]])
    assert (mean, largest) == (0.375, 0.75)
    # three columns of weights 10, 20, 10: overall (0.5, 0.5); tv = 0.5, 0, 0.5
    mean, largest = unfairness([[10, 10, 0], [0, 10, 10]])
    assert (mean, largest) == (0.25, 0.5)
    # an empty column takes no part: overall (0.25, 0.75); columns (0.5, 0.5) and (0, 1), both 0.25 away
    assert unfairness([[5, 0, 0], [5, 0, 10]]) == (0.25, 0.25)
    rng = np.random.default_rng(3)
    for _ in range(5):
        counts = rng.integers(0, 9, (rng.integers(2, 10), rng.integers(2, 10)))
        counts[0] += 1
        assert E.unfairness_from_counts(counts) == P.unfairness(counts)


def test_unfairness_refuses_an_empty_matrix():
    for bad in (np.zeros((0, 3)), np.zeros((2, 2)), np.zeros(4)):
        with pytest.raises(ValueError, match="counts must be"):
            E.unfairness_from_counts(bad)


def test_fairness_aggregates_and_key_names():
    rng = np.random.default_rng(4)
    K = 3
    counts = {(i, j): rng.integers(1, 9, (K + i, 4 + j)) for i in range(K) for j in range(K) if i != j}
    got = E.fairness_from_counts(counts, K)
    assert set(got) == {"mean_unfairness_matrix", "max_unfairness_matrix", "mean_unfairness", "max_unfairness",
                        "mean_unfairness_per_target", "mean_unfairness_per_sensitive"}
    assert got["mean_unfairness_matrix"].shape == got["max_unfairness_matrix"].shape == (K, K)
    assert not np.diag(got["mean_unfairness_matrix"]).any() and not np.diag(got["max_unfairness_matrix"]).any()
    for (i, j), c in counts.items():
        assert (got["mean_unfairness_matrix"][i, j], got["max_unfairness_matrix"][i, j]) == P.unfairness(c)
    want = P.fairness_aggregates(got["mean_unfairness_matrix"], got["max_unfairness_matrix"])
    for key, value in want.items():
        assert np.allclose(got[key], value, rtol=0, atol=1e-15), key
    assert type(got["mean_unfairness"]) is float and type(got["max_unfairness"]) is float


# ---- 3. intervened rows -------------------------------------------------------------------------------------------------------
def test_intervened_rows_against_the_factor_table():
    sizes = P.SMALL
    factors = P.factor_table(sizes)
    assert factors.shape == (60, 3) and [tuple(f) for f in factors[:6]] == [(0, 0, 0), (0, 0, 1), (0, 0, 2), (0, 0, 3), (0, 0, 4), (0, 1, 0)]
    base = np.array([0, 59, 17, 17, 33, 5, 42], np.int64)               # with a repeat
    for j, (stride, size) in enumerate(zip(P.strides(sizes), sizes)):
        got = E.intervened_rows(torch.from_numpy(base), stride, size).numpy()
        assert got.dtype == np.int64 and got.shape == (size, len(base))
        assert np.array_equal(got, P.intervened(base, sizes, j))
        for c in range(size):                                            # factor j is c, the others are the base row's
            assert (factors[got[c], j] == c).all()
            others = [k for k in range(3) if k != j]
            assert np.array_equal(factors[got[c]][:, others], factors[base][:, others])
        assert got.min() >= 0 and got.max() < 60


# ---- 4. the downstream aggregates and every key name ----------------------------------------------------------------------------
def test_downstream_aggregates_and_key_names():
    sizes, K = [10, 1000, 100], 3                                        # the order given, not sorted
    rng = np.random.default_rng(5)
    acc_train, acc_test = rng.random((3, K)), rng.random((3, K))
    got = E.downstream_task_aggregates(sizes, acc_train, acc_test)
    assert set(got) == P.downstream_keys(sizes, K)
    assert "1000:efficiency" not in got and {"10:efficiency", "100:efficiency"} <= set(got)
    assert set(P.downstream_keys([10, 100], 2)) == {
        "10:mean_train_accuracy", "10:mean_test_accuracy", "10:min_train_accuracy", "10:min_test_accuracy",
        "10:train_accuracy_factor_0", "10:train_accuracy_factor_1", "10:test_accuracy_factor_0", "10:test_accuracy_factor_1",
        "10:efficiency",
        "100:mean_train_accuracy", "100:mean_test_accuracy", "100:min_train_accuracy", "100:min_test_accuracy",
        "100:train_accuracy_factor_0", "100:train_accuracy_factor_1", "100:test_accuracy_factor_0", "100:test_accuracy_factor_1"}
    want = P.downstream_aggregates(sizes, acc_train, acc_test)
    for key in want:
        assert abs(got[key] - want[key]) <= 1e-15, key
        assert type(got[key]) is float
    assert got["10:efficiency"] == got["10:mean_test_accuracy"] / got["1000:mean_test_accuracy"]
    assert got["100:min_test_accuracy"] == acc_test[2].min() and got["10:train_accuracy_factor_2"] == acc_train[0, 2]
    zero = E.downstream_task_aggregates([10, 100], np.zeros((2, K)), np.zeros((2, K)))
    assert zero["10:efficiency"] == 0.0                                  # 0 / 0 counts as 0
    json.dumps(got)                                                      # Python values: the log takes them as they are


def test_explicitness_key_names():
    got = E.explicitness_from_aucs([1.0, 0.5], [0.75, 0.25])
    assert set(got) == {"explicitness_train", "explicitness_test", "explicitness_train_per_factor", "explicitness_test_per_factor"}
    assert got["explicitness_train"] == 0.75 and got["explicitness_test"] == 0.5


def test_exports_and_log_names():
    for name in ("downstream_task_from_table", "fairness_from_table", "explicitness_from_table"):
        assert name in disvae_amd.__all__ and getattr(disvae_amd, name) is getattr(E, name)
    assert (E.DOWNSTREAM_TASK_FILE, E.FAIRNESS_FILE, E.EXPLICITNESS_FILE) == ("downstream_task.log", "fairness.log", "explicitness.log")


# ---- 5. argument errors, before any device work ---------------------------------------------------------------------------------
def _no_device_work(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("device work before the refusal")
    for mod in (_dcilib, _udrlib, _lib):
        monkeypatch.setattr(mod, "lib", boom)
    monkeypatch.setattr(E, "_stream", boom)
    monkeypatch.setattr(E, "_BoostedFactor", boom)


def test_every_argument_check_raises_before_any_device_work(monkeypatch):
    _no_device_work(monkeypatch)
    t = torch.zeros(60, 4)
    sizes = (3, 4, 5)
    nan = t * float("nan")
    V, G = ValueError, _lib.DvaeHipError
    down = dict(n_train=(10, 30), n_test=20)
    for mean, lat_sizes, kw, exc, text in [
            (torch.zeros(60), sizes, down, V, r"\[N, D\] table"),
            (t, (), down, V, "positive sizes"),
            (t, (3, 0, 5), down, V, "positive sizes"),
            (torch.zeros(600, 4), (2, 300), down, V, "at most 256 classes"),
            (t, sizes, dict(n_train=10, n_test=20), V, "sequence of training-set sizes"),
            (t, sizes, dict(n_train=(), n_test=20), V, "one size or more"),
            (t, sizes, dict(n_train=(10, 10), n_test=20), V, "each once"),
            (t, sizes, dict(n_train=(10, 0), n_test=20), V, "n_train must lie"),
            (t, sizes, dict(n_train=(10, _dcilib.MAX_ROWS + 1), n_test=20), V, "n_train must lie"),
            (t, sizes, dict(n_train=(10, 30), n_test=0), V, "n_test"),
            (t, sizes, dict(n_train=(10, 41), n_test=20), V, r"at most 60 \(rows are drawn without replacement\), got 41 \+ 20"),
            (t, sizes, dict(n_stages=0, **down), V, "n_stages"),
            (t, sizes, dict(n_stages=_dcilib.MAX_STAGES + 1, **down), V, "n_stages"),
            (t, sizes, dict(seed="x", **down), V, "invalid literal"),
            (torch.zeros(60, 65), sizes, down, V, "between 1 and 64"),
            (torch.zeros(59, 4), sizes, down, V, "does not enumerate"),
            (t, sizes, dict(rows=[list(range(30))], **down), V, "one selection per size"),
            (t, sizes, dict(rows=[list(range(30)), list(range(49))], **down), V, r"n_train \+ n_test = 50"),
            (t, sizes, dict(rows=[list(range(30)), [60] * 50], **down), V, "rows must hold"),
            (nan, sizes, down, V, "NaN or an infinity"),
            (t, sizes, down, G, "downstream_task_from_table needs the table on the GPU")]:
        with pytest.raises(exc, match=text):
            E.downstream_task_from_table(mean, lat_sizes, **kw)
    fair = dict(n_train=40, n_test_per_value=5)
    for mean, lat_sizes, kw, exc, text in [
            (torch.zeros(60), sizes, fair, V, r"\[N, D\] table"),
            (t, (3, 0, 5), fair, V, "positive sizes"),
            (torch.zeros(600, 4), (2, 300), fair, V, "at most 256 classes"),
            (t, (60,), fair, V, "two factors of variation or more"),
            (t, sizes, dict(n_train=0, n_test_per_value=5), V, "n_train must lie"),
            (t, sizes, dict(n_train=_dcilib.MAX_ROWS + 1, n_test_per_value=5), V, "n_train must lie"),
            (t, sizes, dict(n_train=61, n_test_per_value=5), V, "n_train must be at most 60"),
            (t, sizes, dict(n_train=40, n_test_per_value=0), V, "n_test_per_value"),
            (t, sizes, dict(n_stages=0, **fair), V, "n_stages"),
            (t, sizes, dict(seed="x", **fair), V, "invalid literal"),
            (torch.zeros(60, 65), sizes, fair, V, "between 1 and 64"),
            (torch.zeros(59, 4), sizes, fair, V, "does not enumerate"),
            (t, sizes, dict(rows=list(range(39)), **fair), V, "n_train = 40"),
            (t, sizes, dict(rows=[60] * 40, **fair), V, "rows must hold"),
            (t, sizes, dict(base_rows=torch.zeros(3, 3, 4, dtype=torch.int64), **fair), V, "base_rows must have shape"),
            (t, sizes, dict(base_rows=torch.full((3, 3, 5), 60), **fair), V, "base_rows must have shape"),
            (nan, sizes, fair, V, "NaN or an infinity"),
            (t, sizes, fair, G, "fairness_from_table needs the table on the GPU")]:
        with pytest.raises(exc, match=text):
            E.fairness_from_table(mean, lat_sizes, **kw)
    assert E.fairness_from_table.__defaults__[:4] == (10000, 100, 0, 100)
    expl = dict(n_train=40, n_test=20)
    for mean, lat_sizes, kw, exc, text in [
            (torch.zeros(60), sizes, expl, V, r"\[N, D\] table"),
            (t, (3, 0, 5), expl, V, "positive sizes"),
            (torch.zeros(600, 4), (2, 300), expl, V, "at most 256 classes"),
            (t, sizes, dict(n_train=0, n_test=20), V, "n_train must lie"),
            (t, sizes, dict(n_train=40, n_test=0), V, "n_test"),
            (t, sizes, dict(n_train=41, n_test=20), V, "without replacement"),
            (t, sizes, dict(seed="x", **expl), V, "invalid literal"),
            (torch.zeros(60, 65), sizes, expl, V, "between 1 and 64"),
            (torch.zeros(59, 4), sizes, expl, V, "does not enumerate"),
            (t, sizes, dict(rows=list(range(59)), **expl), V, r"n_train \+ n_test"),
            (t, sizes, dict(rows=[60] * 60, **expl), V, "rows must hold"),
            (nan, sizes, expl, V, "NaN or an infinity"),
            (t, sizes, expl, G, "explicitness_from_table needs the table on the GPU")]:
        with pytest.raises(exc, match=text):
            E.explicitness_from_table(mean, lat_sizes, **kw)
    for fn in (E.downstream_task_from_table, E.fairness_from_table, E.explicitness_from_table):
        with pytest.raises(TypeError):
            fn(t, sizes, n_bins=20)


class _Loader:
    def __init__(self, n, lat_sizes=None):
        self.dataset = list(range(n))
        if lat_sizes is not None:
            self.dataset = type("Factors", (list,), {"lat_sizes": np.array(lat_sizes), "lat_names": tuple("abc")})(range(n))

    def __iter__(self):
        raise AssertionError("the loader was walked")


def test_evaluator_checks_before_it_encodes(monkeypatch):
    """The three compute_* run through compute_dci's prologue: the same errors with the same messages, nothing encoded."""
    _no_device_work(monkeypatch)

    class _Model(torch.nn.Module):
        latent_dim = 3

        def encoder(self, x):
            raise AssertionError("the encoder ran")
    model = _Model()
    ev = E.Evaluator(model, None, is_progress_bar=False)
    model.train()
    factors = ("Dataset needs to have known true factors of variations to compute the metric. This does not seem to be the case for list")
    enum = "data set of 59 images does not enumerate lat_sizes=[3, 4, 5]"
    cases = [
        ("compute_downstream_task", dict(n_train=(10, 30), n_test=20),
         [(dict(n_train=(10, 41), n_test=20), "n_train + n_test must be at most 60 (rows are drawn without replacement), got 41 + 20"),
          (dict(n_train=(10, 30), n_test=20, n_stages=0), "n_stages must lie in [1, 1024], got 0"),
          ({}, "n_train + n_test must be at most 60 (rows are drawn without replacement), got 10 + 5000")]),
        ("compute_fairness", dict(n_train=40, n_test_per_value=5),
         [(dict(n_train=61), "n_train must be at most 60 (rows are drawn without replacement), got 61"),
          (dict(n_train=40, n_stages=1025), "n_stages must lie in [1, 1024], got 1025"),
          ({}, "n_train must be at most 60 (rows are drawn without replacement), got 10000")]),
        ("compute_explicitness", dict(n_train=40, n_test=20),
         [(dict(n_train=50, n_test=20), "n_train + n_test must be at most 60 (rows are drawn without replacement), got 50 + 20"),
          (dict(n_train=40, n_test=0), "n_test must be at least 1, got 0"),
          ({}, "n_train + n_test must be at most 60 (rows are drawn without replacement), got 10000 + 5000")])]
    for method, good, bad in cases:
        with pytest.raises(ValueError) as e:
            getattr(ev, method)(_Loader(60), **good)
        assert str(e.value) == factors
        with pytest.raises(ValueError) as e:
            getattr(ev, method)(_Loader(59, (3, 4, 5)), **good)
        assert str(e.value) == enum
        for kw, message in bad:
            with pytest.raises(ValueError) as e:
                getattr(ev, method)(_Loader(60, (3, 4, 5)), **kw)
            assert str(e.value) == message
        with pytest.raises(TypeError):
            getattr(ev, method)(_Loader(60, (3, 4, 5)), n_bins=3)
        assert model.training
    for flag in ("is_downstream", "is_fairness", "is_explicitness"):     # the defaults ask for more rows than 60
        with pytest.raises(ValueError):
            ev(_Loader(60, (3, 4, 5)), is_losses=False, **{flag: True})


def test_call_writes_the_three_logs_and_nothing_new_by_default(monkeypatch, tmp_path):
    import os
    ev = E.Evaluator(torch.nn.Linear(1, 1), None, is_progress_bar=False, save_dir=str(tmp_path))
    seen = []

    def canned(name, result):
        def compute(loader, **kw):
            seen.append((name, kw))
            return result
        return compute
    results = {"compute_downstream_task": {"10:mean_test_accuracy": 0.5, "n_train": [10, 100]},
               "compute_fairness": {"mean_unfairness": 0.25, "mean_unfairness_matrix": np.array([[0.0, 0.5], [0.0, 0.0]])},
               "compute_explicitness": {"explicitness_test": 0.75, "explicitness_test_per_factor": np.array([0.5, 1.0])},
               "compute_losses": {"loss": 1.0}}
    for name, result in results.items():
        monkeypatch.setattr(ev, name, canned(name, result))
    loader = object()
    ev(loader)
    assert os.listdir(tmp_path) == ["test_losses.log"] and [s[0] for s in seen] == ["compute_losses"]
    del seen[:]
    ev(loader, is_losses=False, is_downstream=True, is_fairness=True, is_explicitness=True, downstream_args=dict(n_test=7),
       fairness_args=dict(n_train=5), explicitness_args=dict(seed=2))
    assert seen == [("compute_downstream_task", dict(n_test=7)), ("compute_fairness", dict(n_train=5)), ("compute_explicitness", dict(seed=2))]
    assert sorted(os.listdir(tmp_path)) == ["downstream_task.log", "explicitness.log", "fairness.log", "test_losses.log"]
    assert json.load(open(tmp_path / "downstream_task.log")) == results["compute_downstream_task"]
    assert json.load(open(tmp_path / "fairness.log")) == {"mean_unfairness": 0.25, "mean_unfairness_matrix": [[0.0, 0.5], [0.0, 0.0]]}
    assert json.load(open(tmp_path / "explicitness.log")) == {"explicitness_test": 0.75, "explicitness_test_per_factor": [0.5, 1.0]}


# ---- 6. explicitness against scikit-learn ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes, n_train, n_test", [(P.SMALL, 40, 20), (P.LARGE, 600, 360)], ids=["N60", "N960"])
def test_explicitness_is_sklearns(sizes, n_train, n_test):
    """fit_logistic_regression(C=1.0) + the rank-sum AUC of its fp32 probabilities against LogisticRegression(C=1.0,
    max_iter=10000, tol=1e-10) + roc_auc_score, on the entangled fixture tables, every factor, train and test rows: within
    EXPLICITNESS_BOUND (the module docstring has the measurement)."""
    from sklearn.linear_model import LogisticRegression                  # the yardstick: no skip without it
    from sklearn.metrics import roc_auc_score
    table = P.entangled_table(sizes)
    rows = P.drawn_rows(len(table), n_train + n_test, 1)
    X = table[rows].astype(np.float64)
    worst = 0.0
    for k, stride in enumerate(P.strides(sizes)):
        values = (rows // stride) % sizes[k]
        classes = np.unique(values[:n_train])
        assert len(classes) == sizes[k]                                  # every value is present: no label is -1
        labels = np.searchsorted(classes, values)
        W, b = E.fit_logistic_regression(X[:n_train], labels[:n_train], len(classes), C=1.0)
        model = LogisticRegression(C=1.0, max_iter=10000, tol=1e-10).fit(X[:n_train], labels[:n_train])
        for part in (slice(0, n_train), slice(n_train, n_train + n_test)):
            ours = P.ovr_auc(E.class_probabilities(W, b, X[part]).to(torch.float32).numpy(), labels[part])[1]
            theirs = model.predict_proba(X[part])
            want = np.mean([roc_auc_score(labels[part] == v, theirs[:, v]) for v in range(len(classes))])
            print("factor %d, %d rows: %.12f against %.12f, difference %.3g" % (k, part.stop - part.start, ours, want, abs(ours - want)))
            worst = max(worst, abs(ours - want))
    print("largest difference %.3g, bound %.3g" % (worst, EXPLICITNESS_BOUND))
    assert worst <= EXPLICITNESS_BOUND


# ---- 7. the preconditions of the GPU tests, from the boosted-tree restatement alone ------------------------------------------------
def restated_accuracies(table, sizes, train, test, n_stages, k):
    """(train accuracy, test accuracy, classes present) of factor k by tests/dci_ref.py, the conventions of dci_from_table"""
    stride = P.strides(sizes)[k]
    v_train, v_test = (train // stride) % sizes[k], (test // stride) % sizes[k]
    classes = np.unique(v_train)
    C = len(classes)
    labels = np.searchsorted(classes, v_train)
    fit = R.fit(table[train], labels, C, n_stages)
    raw = R.predict(table[test], fit["feature"], fit["stats"], np.tile(R.prior(labels, C), (len(test), 1)))
    return (float((classes[R.classes_of(fit["raw"], C)] == v_train).mean()), float((classes[R.classes_of(raw, C)] == v_test).mean()), C)


def test_preconditions_of_the_ideal_table():
    """What the GPU test relies on, by the restatement: on the ideal N = 60 table a draw of 10 rows misses a value of a factor
    and its test accuracy is below 1, a draw of 40 holds every value and predicts every factor of the 20 other rows."""
    sizes, table = P.SMALL, P.ideal_table(P.SMALL)
    seen = {}
    for n in (10, 40):
        rows = P.drawn_rows(60, n + 20, n)
        seen[n] = [restated_accuracies(table, sizes, rows[:n], rows[n:], 10, k) for k in range(3)]
    assert [c for _a, _b, c in seen[40]] == list(sizes) and all(a == 1.0 and b == 1.0 for a, b, _c in seen[40])
    assert [c for _a, _b, c in seen[10]] != list(sizes) and min(b for _a, b, _c in seen[10]) < 1.0
    # with every row in the fit every row is predicted as its own value: what makes the unfairness of the ideal table exactly 0
    every = np.arange(60)
    assert all(restated_accuracies(table, sizes, every, every, 10, k)[:2] == (1.0, 1.0) for k in range(3))


def test_boosted_accuracies_within_the_hull_of_eight_sklearn_seeds():
    """The rule of test_dci_host.py for the accuracies of the downstream task: the restatement's train and test accuracy of every
    factor of the entangled N = 960 table, 100 and 400 training rows, 10 stages, inside the min-max hull of
    GradientBoostingClassifier(n_estimators=10, random_state = 0 .. 7) widened by 25 % of its width, never by less than 1e-12."""
    from sklearn import ensemble                                         # the yardstick: no skip without it
    sizes, table = P.LARGE, P.entangled_table(P.LARGE)
    for n in (100, 400):
        rows = P.drawn_rows(960, n + 200, n)
        train, test = rows[:n], rows[n:]
        for k, stride in enumerate(P.strides(sizes)):
            got = np.array(restated_accuracies(table, sizes, train, test, 10, k)[:2])
            v_train, v_test = (train // stride) % sizes[k], (test // stride) % sizes[k]
            seeds = []
            for seed in range(8):
                model = ensemble.GradientBoostingClassifier(n_estimators=10, random_state=seed).fit(table[train], v_train)
                seeds.append((model.score(table[train], v_train), model.score(table[test], v_test)))
            lo, hi = np.min(seeds, axis=0), np.max(seeds, axis=0)
            widen = np.maximum(0.25 * (hi - lo), 1e-12)
            print("n = %d, factor %d: %s, hull %s .. %s" % (n, k, got, lo, hi))
            assert ((got >= lo - widen) & (got <= hi + widen)).all(), (n, k, got, lo, hi)
