"""-m gpu: the linear-SVM library (lib_more/libdvae_sap_hip.so, csrc/svm_1d.hip; Evaluator.compute_sap_discrete) against the fp64
restatement of tests/sap_ref.py.

The shapes are the smallest at which the kernels can go wrong (CASES): 7 training rows with two classes; 60 rows drawn WITH
repeats from a 30-row table; S = 255 / 256 / 257 around the workgroup's 256 threads (a thread with no row, one row each, one thread
with two) and 1 025 (four rows per thread and one thread with a fifth); D = 1 and D = 3; K = 1 and K = 3 with sizes (2, 3, 5); a
40-class factor; a 256-class factor of which the training rows miss values (K = 1, the class limit); a constant column; the
project's offset family (30 + 1e-3 noise); a separable table with a wide gap (few active rows at the optimum) and pure noise
(every row active).  C is 0.01, the score's own, where the case has rows enough for more than one Newton step at it; the smaller
cases take C = 1 to 100, or the regulariser alone would hold every row active and every fit would stop after its first step.
There is no LDS / workspace switch: more than DVAE_SAP_MAX_ROWS rows are refused (tests/test_sap_host.py), and the case of exactly
DVAE_SAP_MAX_ROWS rows (two classes, D = 1; 82 368 bytes of dynamic LDS, above the 64 KiB a launch gets without asking) is the
accepted side of that refusal.
HALVINGS.  On columns drawn from a continuous distribution the restatement never halves a step.  It does where
a row lies exactly ON the hinge at the optimum, which small dyadic tables arrange: the hinge family (sap_ref.HINGE_COLUMN; 5 rows,
and the same rows 60 times over with C / 60, which is the same objective on more rows than the workgroup has threads).  There the
problem of class 0 takes all 30 halvings and leaves through "nothing along the step lowers the objective"; the test asserts that
the restatement does, and holds the device to the same bounds.  Its iteration count is compared only where no row is on the hinge.

Tolerance.  B of sap_ref.bound, per problem, from the restatement's own point; the device passes at 4 B on (w, b) and at
4 B ||H|| on the gradient at ITS OWN point (evaluated by the restatement) -- both fixed before the first run.  Counts and predicted
classes are compared integer for integer with the restatement's on the device's own coefficients.  Every ratio is printed."""
import functools
import json
import logging
import os

import numpy as np
import pytest
import torch

import sap_ref as R
from gpu_util import DEV, stream
from guard_util import Guarded, run_contract
from disvae_amd import _saplib, Evaluator, sap_discrete_from_score_matrix, sap_discrete_from_table

pytestmark = pytest.mark.gpu
# (name, family, lat_sizes, D, training rows, test rows, rows drawn with repeats, seed, C)
CASES = [
    ("two-classes-7", "noisy", (2, 3, 5), 3, 7, 23, False, 1, 1.0),
    ("repeats-60", "noisy", (2, 3, 5), 3, 60, 30, True, 2, 1.0),
    ("threads-255", "sharp", (2, 3, 50), 3, 255, 45, False, 3, 1.0),
    ("threads-256", "noisy", (2, 3, 50), 1, 256, 44, False, 4, 0.01),
    ("threads-257", "noisy", (2, 3, 50), 3, 257, 43, False, 5, 10.0),
    ("ragged-1025-40-classes", "sharp", (3, 40, 10), 3, 1025, 175, False, 6, 0.01),
    ("one-factor-256-classes", "noisy", (256,), 1, 200, 56, False, 7, 0.01),
    ("constant-column", "constant", (3, 4, 25), 3, 257, 43, False, 8, 1.0),
    ("offset", "offset", (2, 3, 50), 3, 257, 43, False, 9, 100.0),
    ("separable", "separable", (2, 3, 50), 3, 256, 44, False, 10, 0.01),
    ("separable-larger-C", "separable", (3, 40, 10), 2, 1025, 175, False, 11, 0.1),
    ("noise-40-classes", "noise", (3, 40, 10), 1, 1025, 175, False, 12, 0.01),
    ("hinge-5-halvings", "hinge", (3, 2), 1, 5, 6, False, 0, 0.5),
    ("hinge-300-halvings", "hinge", (3, 2), 2, 300, 6, False, 0, 0.5 / 60),
    ("max-rows-two-classes", "noisy", (2, 64, 160), 1, _saplib.MAX_ROWS, 1000, False, 13, 0.01),      # factor 0 alone: K = 1
]
HALVING_CASES = ["hinge-5-halvings", "hinge-300-halvings"]
IDS = [c[0] for c in CASES]


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype).contiguous()


@functools.lru_cache(maxsize=None)
def case(name):
    """The inputs of a case and the restatement's outputs, computed once."""
    _n, family, sizes, D, S, T, repeats, seed, C = CASES[IDS.index(name)]
    tab = R.table(family, sizes, D, seed=seed)
    N = tab.shape[0]
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, N, S + T) if repeats else rng.permutation(N)[:S + T]
    if family == "hinge":
        rows = np.concatenate([np.tile(R.HINGE_ROWS, S // 5), np.arange(T)])
    train, test = rows[:S].astype(np.int64), rows[S:].astype(np.int64)
    lt, le, n = R.labels_of(train, test, sizes)
    if name.startswith("max-rows"):                                          # the C-ABI takes any labels: the first factor alone
        sizes, lt, le, n = sizes[:1], lt[:1], le[:1], n[:1]
        assert n == [2] and S == _saplib.MAX_ROWS and 8 * 56 + 5 * S > 64 * 1024
    coef, its, halvings = R.fit(tab, train, lt, n, C)
    return dict(tab=tab, N=N, D=D, K=len(sizes), S=S, T=T, C=C, train=train, test=test, lt=lt, le=le, n=n, P=len(R.problem_list(n)),
                coef=coef, its=its, halvings=halvings)


def run_fit(c, fill=float("nan")):
    """dvae_sap_fit on poisoned outputs -> (coef [D, P, 2], iterations [D, P]) as numpy."""
    assert c["train"].min() >= 0 and c["train"].max() < c["N"] and c["lt"].min() >= 0        # the kernels trust these
    assert all(c["lt"][j].max() == c["n"][j] - 1 for j in range(c["K"])) and c["S"] <= _saplib.MAX_ROWS
    td, rd, ld = _dev(c["tab"], torch.float32), _dev(c["train"], torch.int64), _dev(c["lt"], torch.int32)
    coef = torch.full((c["D"], c["P"], 2), fill, dtype=torch.float64, device=DEV)
    its = torch.full((c["D"], c["P"]), -7, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    _saplib.call("dvae_sap_fit", td.data_ptr(), rd.data_ptr(), ld.data_ptr(), _saplib.host_classes(c["n"]), c["N"], c["D"], c["K"], c["S"],
                 c["C"], coef.data_ptr(), its.data_ptr(), stream())
    torch.cuda.synchronize()
    return coef.cpu().numpy(), its.cpu().numpy()


def run_accuracy(c, coef, rows, labels, with_predicted=True):
    td, rd, ld, cd = _dev(c["tab"], torch.float32), _dev(rows, torch.int64), _dev(labels, torch.int32), _dev(coef, torch.float64)
    correct = torch.full((c["D"], c["K"]), -7, dtype=torch.int32, device=DEV)
    predicted = torch.full((c["D"], c["K"], len(rows)), -7, dtype=torch.int32, device=DEV) if with_predicted else None
    _saplib.call("dvae_sap_accuracy", td.data_ptr(), rd.data_ptr(), ld.data_ptr(), _saplib.host_classes(c["n"]), c["N"], c["D"], c["K"],
                 len(rows), cd.data_ptr(), correct.data_ptr(), None if predicted is None else predicted.data_ptr(), stream())
    torch.cuda.synchronize()
    return correct.cpu().numpy(), None if predicted is None else predicted.cpu().numpy()


@functools.lru_cache(maxsize=None)
def device_fit(name):
    return run_fit(case(name))


def ratios(tab, train, lt, n, C, coef, its, ref_coef, ref_its):
    """(worst |d theta| / B, worst |gradient at the device's point| / (B ||H||), problems with no row on the hinge, those of them
    whose iteration count is the restatement's)."""
    worst_theta = worst_grad = 0.0
    compared = same = 0
    for d in range(tab.shape[1]):
        x = tab[train, d].astype(np.float64)
        for p, (j, k) in enumerate(R.problem_list(n)):
            pos = lt[j] == k
            cp, cn = R.weights(pos, n[j], C)
            w, b = ref_coef[d, p]
            B, normH = R.bound(x, pos, cp, cn, w, b)
            worst_theta = max(worst_theta, float(np.abs(coef[d, p] - ref_coef[d, p]).max()) / B)
            g = R.gradient(x, pos, cp, cn, coef[d, p, 0], coef[d, p, 1])            # the device's own point, verified
            worst_grad = max(worst_grad, float(np.abs(g).max()) / (B * normH))
            if its is not None and not R.near_hinge(x, pos, w, b, 4 * B):
                compared += 1
                same += int(its[d, p] == ref_its[d, p])
    return worst_theta, worst_grad, compared, same


# ---- 1. the fit against the restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", IDS)
def test_fit_vs_fp64(name):
    c = case(name)
    coef, its = device_fit(name)
    assert coef.shape == c["coef"].shape and np.isfinite(coef).all() and (its >= 1).all() and (c["its"] >= 1).all()
    worst_theta, worst_grad, compared, same = ratios(c["tab"], c["train"], c["lt"], c["n"], c["C"], coef, its, c["coef"], c["its"])
    print("%s: %d problems of %d rows; worst |d theta| %.3f B, worst gradient %.3f B ||H|| (both pass at 4); Newton steps at most %d "
          "(restatement %d), equal on %d of the %d problems with no row on the hinge; halvings in the restatement: %d"
          % (name, c["D"] * c["P"], c["S"], worst_theta, worst_grad, its.max(), c["its"].max(), same, compared, c["halvings"].sum()))
    if name in HALVING_CASES:                                                # class 0 of factor 0: every halving, then the exit that keeps the point
        assert c["halvings"][:, 0].min() == _saplib.MAX_HALVINGS + 1 and c["halvings"][:, 1:].max() == 0 and compared < c["D"] * c["P"]
    else:
        assert c["halvings"].sum() == 0
    assert worst_theta <= 4.0, (name, worst_theta)
    assert worst_grad <= 4.0, (name, worst_grad)
    assert same == compared, (name, same, compared)


@pytest.mark.parametrize("name", IDS)
def test_counts_and_predicted_classes_on_the_devices_own_coefficients(name):
    c = case(name)
    coef, _its = device_fit(name)
    for rows, labels in ((c["train"], c["lt"]), (c["test"], c["le"])):
        correct, predicted = run_accuracy(c, coef, rows, labels)
        want_correct, want_predicted = R.accuracy(c["tab"], rows, labels, c["n"], coef)
        assert np.array_equal(predicted, want_predicted) and np.array_equal(correct, want_correct)
        only_counts, none = run_accuracy(c, coef, rows, labels, with_predicted=False)
        assert none is None and np.array_equal(only_counts, correct)
    if name.startswith("one-factor-256"):
        assert c["n"][0] < 256 and (c["le"] == -1).any()                      # values the training rows miss: errors, whatever is predicted
    if name.startswith("two-classes"):
        assert 2 in c["n"]


def test_ties_go_to_the_lowest_class_and_no_fused_multiply_add():
    from fractions import Fraction
    c = dict(case("threads-256"))
    n = c["n"]
    assert n[:2] == [2, 3] and n[2] >= 3 and c["D"] == 1
    tab = c["tab"].copy()
    tab[:, 0] = np.float32(1.0 + 2.0 ** -23)                                 # every row the same x
    x, w = float(tab[0, 0]), 1.0 + 2.0 ** -30                               # w x = 1 + 2^-23 + 2^-30 + 2^-53: rounds DOWN, to an even last bit
    b = -(w * x)
    assert w * x + b == 0.0 and Fraction(w) * Fraction(x) + Fraction(b) == Fraction(1, 2 ** 53)      # rounded: 0; fused: > 0
    coef = np.zeros((1, c["P"], 2))                                          # two classes: 0 is not > 0 -> class 0
    coef[0, 1:4] = [[1.0, 0.0], [1.0, 0.0], [0.5, 0.0]]                      # three classes: 0 and 1 tie above class 2 -> class 0
    coef[0, 5] = w, b                                                        # class 1 of the last factor ties with class 0 at 0 -> class 0
    c["tab"] = tab
    correct, predicted = run_accuracy(c, coef, c["train"], c["lt"])
    want_correct, want_predicted = R.accuracy(tab, c["train"], c["lt"], n, coef)
    assert (predicted == 0).all()
    assert np.array_equal(predicted, want_predicted) and np.array_equal(correct, want_correct)
    coef[0, 5, 1] = np.nextafter(b, 1.0)                                     # one ulp more: class 1 wins
    _correct, predicted = run_accuracy(c, coef, c["train"], c["lt"])
    assert (predicted[0, 2] == 1).all() and (predicted[0, :2] == 0).all()


# ---- 2. determinism, memory ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["two-classes-7", "ragged-1025-40-classes", "offset", "max-rows-two-classes"] + HALVING_CASES)
def test_same_bits_twice_with_poisoned_outputs(name):
    c = case(name)
    a, ia = device_fit(name)
    b, ib = run_fit(c, fill=-1e300)
    assert a.tobytes() == b.tobytes() and ia.tobytes() == ib.tobytes()


def _call(name):
    return lambda args: _saplib.call(name, *[a.ptr if isinstance(a, Guarded) else a for a in args])


@pytest.mark.parametrize("name", ["two-classes-7", "threads-257", "ragged-1025-40-classes", "one-factor-256-classes"] + HALVING_CASES)
def test_memory_contract(name):
    """Guards untouched, inputs unchanged, every output element written, bits equal to the run on plain tensors whatever the
    surroundings hold (NaN at 256-byte alignment; -1e30 at the weakest alignment promised: the element's own)."""
    c = case(name)
    cls = _saplib.host_classes(c["n"])

    def build_fit(al):
        return [al.inp("table", c["tab"], align=4), al.inp("rows", torch.from_numpy(c["train"]), align=8),
                al.inp("labels", torch.from_numpy(c["lt"]), align=4), cls, c["N"], c["D"], c["K"], c["S"], c["C"],
                al.out("coef", (c["D"], c["P"], 2), dtype=torch.float64, align=8), al.out("iterations", (c["D"], c["P"]), dtype=torch.int32, align=4),
                stream()]
    runs = run_contract("dvae_sap_fit", build_fit, fn=_call("dvae_sap_fit"))
    coef, _its = device_fit(name)
    assert runs[0].args[3].t.cpu().numpy().tobytes() == coef.tobytes()

    def build_acc(al):
        return [al.inp("table", c["tab"], align=4), al.inp("rows", torch.from_numpy(c["test"]), align=8),
                al.inp("labels", torch.from_numpy(c["le"]), align=4), cls, c["N"], c["D"], c["K"], c["T"],
                al.inp("coef", torch.from_numpy(coef), align=8, dtype=torch.float64),
                al.out("correct", (c["D"], c["K"]), dtype=torch.int32, align=4),
                al.out("predicted", (c["D"], c["K"], c["T"]), dtype=torch.int32, align=4), stream()]
    runs = run_contract("dvae_sap_accuracy", build_acc, fn=_call("dvae_sap_accuracy"))
    want_correct, want_predicted = R.accuracy(c["tab"], c["test"], c["le"], c["n"], coef)
    assert np.array_equal(runs[0].args[4].t.cpu().numpy(), want_correct) and np.array_equal(runs[0].args[5].t.cpu().numpy(), want_predicted)


# ---- 3. end to end ------------------------------------------------------------------------------------------------------------------
GRID = R.GRID


def _assert_matches_restatement(got, tab, train, test, C=0.01):
    lt, le, n = R.labels_of(train, test, GRID)
    coef = got["coef"]
    ref_coef, ref_its, _hv = R.fit(tab, train, lt, n, C)
    assert coef.shape == ref_coef.shape
    for rows, labels, key in ((train, lt, "score_matrix_train"), (test, le, "score_matrix")):
        correct, _ = R.accuracy(tab, rows, labels, n, coef)
        assert np.array_equal(got[key], correct / float(len(rows))), key      # the device's counts on its own coefficients, exactly
    assert got["sap_discrete"] == R.sap(got["score_matrix"]) == sap_discrete_from_score_matrix(got["score_matrix"])
    worst_theta, worst_grad, _compared, _same = ratios(tab, train, lt, n, C, coef, None, ref_coef, ref_its)
    assert worst_theta <= 4.0 and worst_grad <= 4.0, (worst_theta, worst_grad)
    assert 1 <= got["n_iterations_max"] <= _saplib.MAX_ITERATIONS
    return worst_theta


def test_from_table_on_ideal_rotated_and_collapsed_tables():
    scores = {}
    rows = R.end_to_end_rows()
    cpu0, dev0 = torch.get_rng_state(), torch.cuda.get_rng_state()
    for name, tab in R.end_to_end_tables().items():
        got = sap_discrete_from_table(_dev(tab, torch.float32), GRID, n_train=240, n_test=120, rows=rows)
        worst = _assert_matches_restatement(got, tab, rows[:240], rows[240:])
        assert got["score_matrix"].shape == got["score_matrix_train"].shape == (6, 4) and got["n_train"] == 240 and got["n_test"] == 120
        assert got["C"] == 0.01 and isinstance(got["sap_discrete"], float) and 1 <= got["n_iterations_max"] <= 20
        scores[name] = got["sap_discrete"]
        print("%s: sap_discrete %.4f, coefficients within %.3f B of the restatement's, at most %d Newton steps"
              % (name, got["sap_discrete"], worst, got["n_iterations_max"]))
    # the thresholds: tests/test_sap_host.py, on the restatement alone (0.427 / 0.113 / 0.033)
    assert scores["ideal"] >= 0.3 and scores["rotated"] <= 0.2 and scores["collapsed"] <= 0.1
    # the seeded selection: the same seed gives the same bits, the global random states are untouched
    td = _dev(R.end_to_end_tables()["ideal"], torch.float32)
    a = sap_discrete_from_table(td, GRID, n_train=200, n_test=100, seed=3)
    b = sap_discrete_from_table(td, GRID, n_train=200, n_test=100, seed=3)
    other = sap_discrete_from_table(td, GRID, n_train=200, n_test=100, seed=4)
    assert torch.equal(torch.get_rng_state(), cpu0) and torch.equal(torch.cuda.get_rng_state(), dev0)
    assert a["coef"].tobytes() == b["coef"].tobytes() and np.array_equal(a["score_matrix"], b["score_matrix"])
    assert a["coef"].tobytes() != other["coef"].tobytes()
    drawn = torch.randperm(360, generator=torch.Generator(device=DEV).manual_seed(3), device=DEV)[:300].cpu().numpy()
    _assert_matches_restatement(a, R.end_to_end_tables()["ideal"], drawn[:200], drawn[200:])
    # one latent: the runner-up counts as 0;  a factor with one value present: no problem, every latent scores alike
    one = sap_discrete_from_table(td[:, :1].contiguous(), GRID, n_train=240, n_test=120, rows=rows)
    assert one["sap_discrete"] == float(one["score_matrix"].mean()) and one["score_matrix"].shape == (1, 4)
    same = np.random.default_rng(6).permutation(120)                         # rows 0 .. 119: factor 0 takes the value 0 only
    flat = sap_discrete_from_table(td, GRID, n_train=80, n_test=40, rows=same)
    assert (flat["score_matrix"][:, 0] == 1.0).all() and flat["coef"].shape == (6, 4 + 5 + 6, 2)
    with pytest.raises(ValueError, match="NaN or an infinity"):
        bad = td.clone()
        bad[7, 2] = float("inf")
        sap_discrete_from_table(bad, GRID, n_train=240, n_test=120)
    with pytest.raises(ValueError, match=r"n_train must lie in \[1, %d\]" % _saplib.MAX_ROWS):
        sap_discrete_from_table(td, GRID, n_train=_saplib.MAX_ROWS + 1, n_test=10, rows=np.zeros(_saplib.MAX_ROWS + 11, dtype=np.int64))


class _TableModel(torch.nn.Module):
    """A model whose encoder looks q(z|x) up in a table: image x is its row number."""

    def __init__(self, mean):
        super().__init__()
        self.latent_dim = mean.shape[1]
        self.register_buffer("mean", torch.from_numpy(np.ascontiguousarray(mean)))
        self.modes = []

    def encoder(self, x):
        self.modes.append(self.training)
        idx = x.view(-1).long()
        return self.mean[idx], torch.zeros_like(self.mean[idx])


class _Factors:
    lat_sizes, lat_names = np.array(GRID), tuple("abcd")

    def __len__(self):
        return 360


class _Loader:
    dataset = _Factors()

    def __iter__(self):
        for lo in range(0, 360, 100):
            yield torch.arange(lo, min(lo + 100, 360), dtype=torch.float32).view(-1, 1), None


def test_evaluator_end_to_end(tmp_path):
    tab = R.end_to_end_tables()["ideal"]
    model = _TableModel(tab).train()
    ev = Evaluator(model, None, device=torch.device(DEV), logger=logging.getLogger("sap"), save_dir=str(tmp_path), is_progress_bar=False)
    kw = dict(n_train=240, n_test=120, seed=2)
    got = ev.compute_sap_discrete(_Loader(), **kw)
    again = ev.compute_sap_discrete(_Loader(), **kw)
    assert model.training and model.modes == [False] * 8                     # encoded in eval mode, mode restored
    assert got["coef"].tobytes() == again["coef"].tobytes() and got["sap_discrete"] == again["sap_discrete"]
    assert np.array_equal(got["score_matrix"], again["score_matrix"])
    direct = sap_discrete_from_table(_dev(tab, torch.float32), GRID, **kw)
    assert direct["coef"].tobytes() == got["coef"].tobytes() and direct["sap_discrete"] == got["sap_discrete"] >= 0.3
    assert ev(_Loader(), is_losses=False) == (None, None) and os.listdir(tmp_path) == []
    assert ev(_Loader(), is_losses=False, is_sap_discrete=True, sap_discrete_args=kw) == (None, None)
    assert os.listdir(tmp_path) == ["sap_discrete.log"]
    logged = json.load(open(tmp_path / "sap_discrete.log"))
    assert set(logged) == set(got) - {"score_matrix", "score_matrix_train", "coef"}
    assert logged["sap_discrete"] == got["sap_discrete"] and logged["n_iterations_max"] == got["n_iterations_max"]
    assert model.training and not any(model.modes)
    with pytest.raises(ValueError, match=r"n_train \+ n_test must be at most 360"):
        ev.compute_sap_discrete(_Loader())                                   # the defaults want 15 000 rows

    class _NoFactors:
        dataset = [0, 1, 2, 3]
    with pytest.raises(ValueError, match="Dataset needs to have known true factors of variations to compute the metric"):
        ev.compute_sap_discrete(_NoFactors())
