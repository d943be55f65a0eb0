"""CPU, no library call: what every Evaluator.compute_* does BEFORE its kernels -- which error a wrong data set or argument
raises (type, full message, and which of two wins), that nothing is encoded before the checks pass, that the encoder runs in
eval mode and train mode comes back (also when the encoder raises), what reaches the *_from_table function -- and what
Evaluator.__call__ logs and writes for every optional output.  A stub model and fake data sets: lat_sizes=[3, 2] with 6 rows, the
same with 5 rows, one without lat_sizes, and the few more that one line of a _check_* function needs."""
import json
import os

import numpy as np
import pytest
import torch

from disvae_amd import evaluate as E

D = 2


class _Model(torch.nn.Module):
    latent_dim = D

    def __init__(self):
        super().__init__()
        self.modes, self.fail = [], False

    def encoder(self, x):
        self.modes.append(self.training)
        if self.fail:
            raise RuntimeError("the encoder failed")
        n = x.shape[0]
        return x[:, :1] + torch.tensor([[0.0, 0.5]]), torch.zeros(n, D)


class _Plain(list):
    pass


class _Factors(list):
    pass


class _Unsized:
    pass


class _Huge:
    def __len__(self):
        return (1 << 23) + 1


def _dataset(rows, lat_sizes=None):
    if lat_sizes is None:
        return _Plain(range(rows))
    ds = _Factors(range(rows))
    ds.lat_sizes, ds.lat_names = np.array(lat_sizes, dtype=np.int64), tuple("abcdefghij"[:len(lat_sizes)])
    return ds


class _Loader:
    """Batches of 4 rows; row r of the data is the number r.  yields: the rows the loader walks, where not len(dataset)."""

    def __init__(self, dataset, yields=None):
        self.dataset = dataset
        self.rows = len(dataset) if yields is None else yields

    def __iter__(self):
        for lo in range(0, self.rows, 4):
            yield torch.arange(lo, min(lo + 4, self.rows), dtype=torch.float32).view(-1, 1), None


def FULL():
    return _Loader(_dataset(6, [3, 2]))


def SHORT():
    return _Loader(_dataset(5, [3, 2]))


def PLAIN():
    return _Loader(_dataset(6))


def YIELDS5():
    return _Loader(_dataset(6, [3, 2]), yields=5)


def sized(rows, lat_sizes):
    return lambda: _Loader(_dataset(rows, lat_sizes), yields=0)


FACTORS = ("Dataset needs to have known true factors of variations to compute the metric. This does not seem to be the case for "
           "_Plain")
ENUM5 = "data set of 5 images does not enumerate lat_sizes=[3, 2]"
LIE = "n_samples must lie in [1, 6] (rows are drawn without replacement) or be None, got %d"
SCORE = dict(n_train=4, n_eval=4, batch_size=2, n_variance=6)
DCI = dict(n_train=4, n_test=2)
V, T = ValueError, TypeError
UNEXPECTED = "() got an unexpected keyword argument 'n_bins'"       # behind the function's name, which Python spells by version

# (method, loader, keyword arguments, exception, full message, was the encoder reached: True / False / None = not pinned)
CASES = [
    # ---- compute_factor_scores / _check_score_sizes
    ("compute_factor_scores", PLAIN, SCORE, V, FACTORS, False),
    ("compute_factor_scores", SHORT, SCORE, V, ENUM5, False),
    ("compute_factor_scores", YIELDS5, SCORE, V, ENUM5, True),
    ("compute_factor_scores", sized(0, [3, 0]), SCORE, V, "lat_sizes must hold positive sizes, got [3, 0]", False),
    ("compute_factor_scores", sized(1, []), SCORE, V, "lat_sizes must hold positive sizes, got []", False),
    ("compute_factor_scores", sized(1, [1, 1]), SCORE, V, "no factor of variation takes two values or more: lat_sizes=[1, 1]", False),
    ("compute_factor_scores", FULL, dict(SCORE, n_train=0), V, "n_train and n_eval must be >= 1, got 0 and 4", False),
    ("compute_factor_scores", FULL, dict(SCORE, n_eval=0), V, "n_train and n_eval must be >= 1, got 4 and 0", False),
    ("compute_factor_scores", FULL, dict(SCORE, batch_size=1), V, "batch_size must be >= 2 (a variance needs two points), got 1", False),
    ("compute_factor_scores", FULL, dict(SCORE, n_variance=1), V,
     "the global variance needs two rows or more: n_variance=1 on 6 images", False),
    ("compute_factor_scores", SHORT, dict(SCORE, n_train=0), V, "n_train and n_eval must be >= 1, got 0 and 4", False),    # doubly wrong
    ("compute_factor_scores", PLAIN, dict(SCORE, batch_size=1), V, FACTORS, False),                                      # doubly wrong
    ("compute_factor_scores", FULL, dict(SCORE, n_train=0, batch_size=1), V, "n_train and n_eval must be >= 1, got 0 and 4", False),
    # ---- compute_information_scores / _check_information_sizes
    ("compute_information_scores", PLAIN, {}, V, FACTORS, False),
    ("compute_information_scores", SHORT, {}, V, ENUM5, False),
    ("compute_information_scores", YIELDS5, {}, V, ENUM5, True),
    ("compute_information_scores", sized(0, [3, 0]), {}, V, "lat_sizes must hold positive sizes, got [3, 0]", False),
    ("compute_information_scores", sized(1, []), {}, V, "lat_sizes must hold positive sizes, got []", False),
    ("compute_information_scores", sized(6, [2] * 9), {}, V, "9 factors of variation: the kernels take at most 8", False),
    ("compute_information_scores", FULL, dict(n_bins=0), V, "n_bins must lie in [1, 64], got 0", False),
    ("compute_information_scores", FULL, dict(n_bins=65), V, "n_bins must lie in [1, 64], got 65", False),
    ("compute_information_scores", sized(3, [3, 1]), {}, V,
     "a factor of variation with one value has no entropy (the MIG divides by it): lat_sizes=[3, 1]", False),
    ("compute_information_scores", FULL, dict(n_samples=7), V, LIE % 7, False),
    ("compute_information_scores", FULL, dict(n_samples=0), V, LIE % 0, False),
    ("compute_information_scores", SHORT, dict(n_bins=0), V, "n_bins must lie in [1, 64], got 0", False),                # doubly wrong
    ("compute_information_scores", SHORT, dict(n_samples=6), V, ENUM5, False),        # n is prod(lat_sizes), not len(ds)
    ("compute_information_scores", FULL, dict(n_bins=0, n_samples=7), V, "n_bins must lie in [1, 64], got 0", False),    # doubly wrong
    ("compute_information_scores", sized(6, [2] * 8 + [0]), {}, V,
     "lat_sizes must hold positive sizes, got [2, 2, 2, 2, 2, 2, 2, 2, 0]", False),                                       # doubly wrong
    # ---- compute_irs / _check_irs_arguments
    ("compute_irs", PLAIN, {}, V, FACTORS, False),
    ("compute_irs", SHORT, {}, V, ENUM5, False),
    ("compute_irs", YIELDS5, {}, V, ENUM5, True),
    ("compute_irs", sized(0, [3, 0]), {}, V, "lat_sizes must hold positive sizes, got [3, 0]", False),
    ("compute_irs", sized(1, []), {}, V, "lat_sizes must hold positive sizes, got []", False),
    ("compute_irs", sized(6, [2] * 9), {}, V, "9 factors of variation: the kernels take at most 8", False),
    ("compute_irs", FULL, dict(diff_quantile=1.5), V, "diff_quantile must lie in [0, 1], got 1.5", False),
    ("compute_irs", FULL, dict(factor_bins=0), V, "factor_bins must be >= 1 or None (every value its own group), got 0", False),
    ("compute_irs", sized(6, [257, 2]), dict(factor_bins=None), V,
     "257 groups of one factor: the kernels take at most 256 (use factor_bins)", False),
    ("compute_irs", sized(6, [257, 2]), dict(factor_bins=300), V,
     "257 groups of one factor: the kernels take at most 256 (use factor_bins)", False),
    ("compute_irs", FULL, dict(n_samples=0), V, LIE % 0, False),
    ("compute_irs", FULL, dict(n_samples=7), V, LIE % 7, False),
    ("compute_irs", SHORT, dict(diff_quantile=-1), V, "diff_quantile must lie in [0, 1], got -1", False),                 # doubly wrong
    ("compute_irs", FULL, dict(factor_bins=0, n_samples=7), V,
     "factor_bins must be >= 1 or None (every value its own group), got 0", False),                                       # doubly wrong
    # ---- compute_dci / _check_dci_arguments
    ("compute_dci", PLAIN, DCI, V, FACTORS, False),
    ("compute_dci", SHORT, DCI, V, ENUM5, False),
    ("compute_dci", YIELDS5, DCI, V, ENUM5, True),
    ("compute_dci", sized(0, [3, 0]), DCI, V, "lat_sizes must hold positive sizes, got [3, 0]", False),
    ("compute_dci", sized(1, []), DCI, V, "lat_sizes must hold positive sizes, got []", False),
    ("compute_dci", sized(6, [257, 2]), DCI, V,
     "a factor of variation with 257 values: the boosted-tree kernels take at most 256 classes", False),
    ("compute_dci", FULL, dict(DCI, n_train=0), V, "n_train must lie in [1, 10240], got 0", False),
    ("compute_dci", FULL, dict(DCI, n_train=10241), V, "n_train must lie in [1, 10240], got 10241", False),
    ("compute_dci", FULL, dict(DCI, n_test=0), V, "n_test must be at least 1, got 0", False),
    ("compute_dci", FULL, dict(DCI, n_stages=0), V, "n_stages must lie in [1, 1024], got 0", False),
    ("compute_dci", FULL, dict(DCI, seed="x"), V, "invalid literal for int() with base 10: 'x'", False),
    ("compute_dci", FULL, dict(n_train=5, n_test=2), V,
     "n_train + n_test must be at most 6 (rows are drawn without replacement), got 5 + 2", False),
    ("compute_dci", FULL, {}, V, "n_train + n_test must be at most 6 (rows are drawn without replacement), got 10000 + 5000", False),
    ("compute_dci", SHORT, dict(DCI, n_stages=0), V, "n_stages must lie in [1, 1024], got 0", False),                     # doubly wrong
    ("compute_dci", FULL, dict(n_train=5, n_test=2, n_stages=0), V, "n_stages must lie in [1, 1024], got 0", False),      # doubly wrong
    ("compute_dci", FULL, dict(DCI, n_bins=3), T, UNEXPECTED, False),
    # ---- compute_metrics (it has no _check_* function; whether 5 of 6 rows are encoded before the error is not pinned)
    ("compute_metrics", PLAIN, {}, V, FACTORS, False),
    ("compute_metrics", SHORT, {}, V, ENUM5, None),
    ("compute_metrics", YIELDS5, {}, V, ENUM5, True),
    # ---- compute_unsupervised_scores / _check_unsupervised_arguments
    ("compute_unsupervised_scores", PLAIN, dict(n_bins=0), V, "n_bins must lie in [1, 64], got 0", False),
    ("compute_unsupervised_scores", PLAIN, dict(n_samples=0), V, "n_samples must be at least 1 or None, got 0", False),
    ("compute_unsupervised_scores", lambda: _Loader(_dataset(0)), {}, V, "the table of means must hold one row or more", False),
    ("compute_unsupervised_scores", PLAIN, dict(n_samples=7), V, LIE % 7, False),
    ("compute_unsupervised_scores", FULL, dict(n_samples=7), V, LIE % 7, False),
    ("compute_unsupervised_scores", PLAIN, dict(n_bins=0, n_samples=0), V, "n_bins must lie in [1, 64], got 0", False),  # doubly wrong
    ("compute_unsupervised_scores", lambda: _Loader(_dataset(0)), dict(n_samples=0), V,
     "n_samples must be at least 1 or None, got 0", False),                                                               # doubly wrong
    # ---- compute_elbo_decomposition (its checks are its own)
    ("compute_elbo_decomposition", PLAIN, dict(n_samples=0), V, "n_samples must be >= 1 (or None for the whole data set), got 0", False),
    ("compute_elbo_decomposition", PLAIN, dict(n_samples=7), V,
     "n_samples=7 exceeds the 6 images of the data set (samples are drawn without replacement)", False),
    ("compute_elbo_decomposition", PLAIN, dict(n_samples=3, eps=torch.zeros(2, D)), V, "eps must have shape (3, 2), got (2, 2)", False),
    ("compute_elbo_decomposition", PLAIN, dict(sample_idx=[0, 6]), V, "sample_idx must hold rows in [0, 6)", False),
    ("compute_elbo_decomposition", lambda: _Loader(_dataset(6), yields=5), dict(n_samples=3), V,
     "the loader yielded 5 images, its data set has 6", True),
    ("compute_elbo_decomposition", PLAIN, dict(n_samples=7, eps=torch.zeros(2, D)), V,
     "n_samples=7 exceeds the 6 images of the data set (samples are drawn without replacement)", False),                  # doubly wrong
    # ---- compute_log_likelihood
    ("compute_log_likelihood", PLAIN, dict(n_samples=0), V, "n_samples must be >= 1, got 0", False),
]
UDR_CASES = [
    (0, PLAIN, {}, V, "UDR compares the models of a sweep: two or more are needed, got 1", False),
    (1, PLAIN, dict(correlation="pearson"), V, "correlation must be one of ('spearman', 'lasso'), got 'pearson'", False),
    (1, PLAIN, dict(n_samples=0), V, "n_samples must be at least 1 or None, got 0", False),
    (1, PLAIN, dict(kl_threshold=-1), V, "kl_threshold must be a finite number >= 0, got -1", False),
    (1, PLAIN, dict(lasso_alpha=float("inf")), V, "lasso_alpha must be a finite number >= 0, got inf", False),
    (1, PLAIN, dict(seed="x"), V, "invalid literal for int() with base 10: 'x'", False),
    (1, lambda: _Loader(_dataset(0)), {}, V, "the tables must hold one row or more", False),
    (1, PLAIN, dict(n_samples=7), V, LIE % 7, False),
    (1, lambda: _Loader(_Huge(), yields=0), {}, V, "UDR ranks at most 8388608 rows: pass n_samples", False),
    (1, PLAIN, dict(n_bins=3), T, UNEXPECTED, False),
    (0, PLAIN, dict(correlation="pearson"), V, "UDR compares the models of a sweep: two or more are needed, got 1", False),   # doubly wrong
    (1, PLAIN, dict(correlation="pearson", n_samples=0), V, "correlation must be one of ('spearman', 'lasso'), got 'pearson'", False),
    (1, lambda: _Loader(_dataset(0)), dict(kl_threshold=-1), V, "kl_threshold must be a finite number >= 0, got -1", False),
]


def _evaluator(**kw):
    model = _Model()
    return E.Evaluator(model, None, is_progress_bar=False, **kw), model


def _ids(cases):
    return ["%s-%d" % (c[0], i) for i, c in enumerate(cases)]


# ---- (a) the errors of every compute_* -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method, loader, kw, exc, message, encoded", CASES, ids=_ids(CASES))
def test_compute_errors_and_their_order(method, loader, kw, exc, message, encoded):
    ev, model = _evaluator()
    model.train()
    with pytest.raises(exc) as e:
        getattr(ev, method)(loader(), **kw)
    assert str(e.value).endswith(message) if exc is T else str(e.value) == message
    assert model.training                                                 # train mode is back
    if encoded is not None:
        assert bool(model.modes) == encoded                               # no check waits for the encoder that could come before it
    if method != "compute_metrics":                                       # (compute_metrics is called in eval mode by __call__)
        assert not any(model.modes)                                       # the encoder only ever ran in eval mode


@pytest.mark.parametrize("n_others, loader, kw, exc, message, encoded", UDR_CASES, ids=_ids(UDR_CASES))
def test_compute_udr_errors_and_their_order(n_others, loader, kw, exc, message, encoded):
    ev, model = _evaluator()
    others = [_Model() for _ in range(n_others)]
    for m in [model] + others:
        m.train()
    with pytest.raises(exc) as e:
        ev.compute_udr(loader(), others, **kw)
    assert str(e.value).endswith(message) if exc is T else str(e.value) == message
    assert all(m.training for m in [model] + others)
    assert not any(m.modes for m in [model] + others)


RAISING = [("compute_factor_scores", FULL, SCORE), ("compute_information_scores", FULL, {}), ("compute_irs", FULL, {}),
           ("compute_dci", FULL, DCI), ("compute_unsupervised_scores", PLAIN, {}), ("compute_elbo_decomposition", PLAIN, dict(n_samples=3))]


@pytest.mark.parametrize("method, loader, kw", RAISING, ids=[r[0] for r in RAISING])
@pytest.mark.parametrize("training", [True, False])
def test_mode_is_restored_when_the_encoder_raises(method, loader, kw, training):
    ev, model = _evaluator()
    model.train(training)
    model.fail = True
    with pytest.raises(RuntimeError, match="^the encoder failed$"):
        getattr(ev, method)(loader(), **kw)
    assert model.training == training and model.modes == [False]


def test_udr_restores_every_model_when_an_encoder_raises():
    ev, model = _evaluator()
    others = [_Model(), _Model()]
    model.train()
    others[0].eval()
    others[1].train()
    others[1].fail = True
    with pytest.raises(RuntimeError, match="^the encoder failed$"):
        ev.compute_udr(PLAIN(), others)
    assert [m.training for m in [model] + others] == [True, False, True]
    assert [m.modes for m in [model] + others] == [[False], [False], [False]]


# ---- what reaches the *_from_table functions -------------------------------------------------------------------------------------
TABLE = torch.arange(6, dtype=torch.float32).view(6, 1) + torch.tensor([[0.0, 0.5]])
PASSED = [
    ("compute_factor_scores", "factor_scores_from_table", FULL, dict(SCORE, seed=3), True,
     dict(SCORE, active_threshold=0.05, seed=3, draws=None)),
    ("compute_information_scores", "information_scores_from_table", FULL, dict(n_samples=6), True, dict(n_bins=20, n_samples=6, seed=0)),
    ("compute_irs", "irs_from_table", FULL, dict(factor_bins=None), True, dict(diff_quantile=0.99, factor_bins=None, n_samples=None, seed=0)),
    ("compute_dci", "dci_from_table", FULL, DCI, True, dict(DCI, seed=0, n_stages=100)),
    ("compute_unsupervised_scores", "unsupervised_scores_from_table", PLAIN, dict(n_bins=5), False, dict(n_bins=5, n_samples=None, seed=0)),
    # a data set that cannot tell its length: n_samples is the table function's to check
    ("compute_unsupervised_scores", "unsupervised_scores_from_table", lambda: _Loader(_Unsized(), yields=6), dict(n_samples=7), False,
     dict(n_bins=20, n_samples=7, seed=0)),
]


@pytest.mark.parametrize("method, target, loader, kw, with_sizes, want_kw", PASSED, ids=["%s-%d" % (p[0], i) for i, p in enumerate(PASSED)])
@pytest.mark.parametrize("training", [True, False])
def test_compute_hands_the_table_on(monkeypatch, method, target, loader, kw, with_sizes, want_kw, training):
    seen = []
    monkeypatch.setattr(E, target, lambda *a, **k: seen.append((a, k)) or "the result")
    ev, model = _evaluator()
    model.train(training)
    assert getattr(ev, method)(loader(), **kw) == "the result"
    (args, got_kw), = seen
    assert got_kw == want_kw and len(args) == (2 if with_sizes else 1)
    assert torch.equal(args[0], TABLE)
    if with_sizes:
        assert args[1] == [3, 2] and all(type(k) is int for k in args[1])
    assert model.training == training and model.modes == [False, False]   # two batches, both in eval mode


def test_compute_udr_hands_the_tables_on(monkeypatch):
    seen = []
    monkeypatch.setattr(E, "udr_from_tables", lambda *a, **k: seen.append((a, k)) or "the result")
    ev, model = _evaluator()
    other = _Model()
    model.train()
    other.eval()
    assert ev.compute_udr(PLAIN(), [other], n_samples=4, correlation="lasso") == "the result"
    ((means, logvars), kw), = seen
    assert kw == dict(n_samples=4, correlation="lasso")
    assert len(means) == len(logvars) == 2 and all(torch.equal(m, TABLE) for m in means)
    assert all(torch.equal(lv, torch.zeros(6, D)) for lv in logvars)
    assert model.training and not other.training and model.modes == other.modes == [False, False]


# ---- (b) Evaluator.__call__ ------------------------------------------------------------------------------------------------------
class _Log:
    def __init__(self):
        self.lines = []

    def info(self, message):
        self.lines.append(message)


def _canned(**extra):
    return dict({"score": 0.5, "count": 3, "vector": np.array([1.0, 2.5]), "matrix": np.array([[1.0, 2.0], [3.0, 4.0]]),
                 "raw_correlations": np.array([0.25, 0.75])}, **extra)


PLAIN_RESULTS = {
    "compute_metrics": {"MIG": 0.25, "AAM": 0.75},
    "compute_losses": {"loss": 1.5, "recon_loss": 1.25},
    "compute_log_likelihood": {"log_likelihood": -90.5, "n_samples": 7, "rec_dist": "bernoulli"},
    "compute_elbo_decomposition": {"H_z": 2.0, "H_z_d": [1.0, 1.5], "mi": 0.5, "n_samples": 11},
    "compute_factor_scores": {"factor_vae_eval": 0.5, "n_active": 2},
}
ARRAY_RESULTS = ["compute_information_scores", "compute_irs", "compute_unsupervised_scores", "compute_udr", "compute_dci"]
LISTED = {"score": 0.5, "count": 3, "vector": [1.0, 2.5]}
WRITTEN = {
    "metrics.log": PLAIN_RESULTS["compute_metrics"],
    "test_losses.log": PLAIN_RESULTS["compute_losses"],
    "log_likelihood.log": PLAIN_RESULTS["compute_log_likelihood"],
    "elbo_decomposition.log": PLAIN_RESULTS["compute_elbo_decomposition"],
    "factor_scores.log": PLAIN_RESULTS["compute_factor_scores"],
    "information_scores.log": dict(LISTED, raw_correlations=[0.25, 0.75], which="compute_information_scores"),
    "irs.log": dict(LISTED, matrix=[[1.0, 2.0], [3.0, 4.0]], raw_correlations=[0.25, 0.75], which="compute_irs"),
    "unsupervised_scores.log": dict(LISTED, raw_correlations=[0.25, 0.75], which="compute_unsupervised_scores"),
    "udr.log": dict(LISTED, matrix=[[1.0, 2.0], [3.0, 4.0]], which="compute_udr"),
    "dci.log": {"score": 0.5, "count": 3, "which": "compute_dci"},
}
MESSAGES = [
    "Computing metrics...",
    "Losses: {'MIG': 0.25, 'AAM': 0.75}",
    "Computing losses...",
    "Losses: {'loss': 1.5, 'recon_loss': 1.25}",
    "Computing the importance-weighted log-likelihood...",
    "Log-likelihood: {'log_likelihood': -90.5, 'n_samples': 7, 'rec_dist': 'bernoulli'}",
    "Computing the ELBO decomposition over the data set...",
    "ELBO decomposition: {'H_z': 2.0, 'H_z_d': [1.0, 1.5], 'mi': 0.5, 'n_samples': 11}",
    "Computing the FactorVAE and beta-VAE scores...",
    "Disentanglement scores: {'factor_vae_eval': 0.5, 'n_active': 2}",
    "Computing the discretised MIG, modularity and SAP scores...",
    "Information scores: {'score': 0.5, 'count': 3, 'vector': [1.0, 2.5], 'raw_correlations': [0.25, 0.75], "
    "'which': 'compute_information_scores'}",
    "Computing the interventional robustness score...",
    "IRS: {'score': 0.5, 'count': 3, 'vector': [1.0, 2.5], 'matrix': [[1.0, 2.0], [3.0, 4.0]], 'raw_correlations': [0.25, 0.75], "
    "'which': 'compute_irs'}",
    "Computing the label-free scores...",
    "Unsupervised scores: {'score': 0.5, 'count': 3, 'vector': [1.0, 2.5], 'raw_correlations': [0.25, 0.75], "
    "'which': 'compute_unsupervised_scores'}",
    "Computing the unsupervised disentanglement ranking...",
    "UDR: {'score': 0.5, 'count': 3, 'vector': [1.0, 2.5], 'matrix': [[1.0, 2.0], [3.0, 4.0]], 'which': 'compute_udr'}",
    "Computing the DCI scores...",
    "DCI: {'score': 0.5, 'count': 3, 'which': 'compute_dci'}",
]


def _canned_evaluator(monkeypatch, save_dir):
    log, calls = _Log(), []
    ev, model = _evaluator(logger=log, save_dir=save_dir)
    assert log.lines == ["Testing Device: cpu"]
    del log.lines[:]

    def canned(name, result):
        def compute(*args, **kw):
            calls.append((name, args, kw, model.training))
            return result
        return compute
    for name, result in PLAIN_RESULTS.items():
        monkeypatch.setattr(ev, name, canned(name, result))
    for name in ARRAY_RESULTS:
        monkeypatch.setattr(ev, name, canned(name, _canned(which=name)))
    return ev, model, log, calls


def test_call_logs_and_writes_every_output(monkeypatch, tmp_path):
    save_dir = str(tmp_path / "results" / "run")                          # __call__ makes the directory
    ev, model, log, calls = _canned_evaluator(monkeypatch, save_dir)
    loader, others = object(), [object()]
    model.train()
    got = ev(loader, is_metrics=True, is_losses=True, is_log_likelihood=True, n_samples=7, is_decomposition=True,
             n_samples_decomposition=11, is_scores=True, is_information=True, is_irs=True, is_unsupervised=True, udr_models=others,
             is_dci=True, dci_args=dict(n_train=4, n_test=2))
    assert got == (None, PLAIN_RESULTS["compute_losses"])                 # the reference's (metric, losses): metric stays None
    assert got[1] is PLAIN_RESULTS["compute_losses"]
    assert model.training
    assert log.lines[:-1] == MESSAGES
    assert log.lines[-1].startswith("Finished evaluating after ") and log.lines[-1].endswith(" min.")
    assert calls == [("compute_metrics", (loader,), {}, False), ("compute_losses", (loader,), {}, False),
                     ("compute_log_likelihood", (loader,), dict(n_samples=7), False),
                     ("compute_elbo_decomposition", (loader,), dict(n_samples=11), False),
                     ("compute_factor_scores", (loader,), {}, False), ("compute_information_scores", (loader,), {}, False),
                     ("compute_irs", (loader,), {}, False), ("compute_unsupervised_scores", (loader,), {}, False),
                     ("compute_udr", (loader, others), {}, False), ("compute_dci", (loader,), dict(n_train=4, n_test=2), False)]
    assert sorted(os.listdir(save_dir)) == sorted(WRITTEN)
    for name, want in WRITTEN.items():
        text = open(os.path.join(save_dir, name)).read()
        assert json.loads(text) == want, name
        assert text == json.dumps(want, indent=4, sort_keys=True), name


def test_call_writes_only_the_losses_by_default(monkeypatch, tmp_path):
    save_dir = str(tmp_path / "results")
    ev, model, log, calls = _canned_evaluator(monkeypatch, save_dir)
    loader = object()
    model.eval()
    assert ev(loader) == (None, PLAIN_RESULTS["compute_losses"])
    assert not model.training
    assert [c[0] for c in calls] == ["compute_losses"]
    assert log.lines[:-1] == MESSAGES[2:4]
    assert os.listdir(save_dir) == ["test_losses.log"]
    # is_dci without dci_args: the defaults; nothing else is computed
    del calls[:], log.lines[:]
    assert ev(loader, is_losses=False, is_dci=True) == (None, None)
    assert calls == [("compute_dci", (loader,), {}, False)] and log.lines[:-1] == MESSAGES[18:]
    assert sorted(os.listdir(save_dir)) == ["dci.log", "test_losses.log"]
