"""-m gpu: the softmax-regression library (lib_scores/libdvae_lr_hip.so, csrc/softmax_fit.hip) through the C-ABI against the fp64
restatement tests/lr_ref.py, and the scores on top of it (fit="device" of explicitness and the beta-VAE score, InfoE) end to end.

The cases are lr_ref.CASES: the smallest shapes at which the kernels can go wrong -- S = 2; 63 / 64 / 65 around the 64 rows of a chunk
of the sums over the rows; 511 / 512 / 513 around the workgroup's threads; DVAE_LR_MAX_ROWS once (D = 2, two classes); D = 1, 10,
17 (two feature tiles, the second ragged) and 64; 2, 3, 40 and 256 classes (256 at S = 512, D = 2: more entries than threads);
Q = 1, 2, 5 and 8 problems of mixed classes; Gaussian features with random labels, a separable factor-aligned table (the penalty
alone keeps its optimum finite: ||H^+|| up to 1e6), the +30 offset family raw and with shift / scale, a constant column (zero, and
5.0 under scale 0: its weights come back exactly 0), duplicate rows, a class with one row.

ACCEPTANCE, derived in lr_ref's docstring and fixed before the first run (tolerance_grad = 1e-8; u = 2^-53):
  g = max |grad f| of the RESTATEMENT at the device's point             <= tolerance_grad + 4 B_g
  || centred(theta_dev) - theta* ||_inf                                 <= 2 ||H(theta*)^+||_inf (tolerance_grad + 4 B_g)
  | report[:, 1] - g |                                                  <= 4 B_g
  f(theta_dev) (restatement)                                            <= f(host fit: fit_logistic_regression) + 4 B_f;  | report[:, 0] - f | <= 4 B_f
B_g is the first-order fp64 rounding bound of the device's gradient sum IN THE ORDER IT ADDS: a term passes the L = ceil(S / n_chunks)
additions of its chunk and the n_chunks additions of the partials, so (L + n_chunks + 1) u sum_i |r_ic x_id| / S, plus the error of
the probabilities (the logit's D + 1 operations, exp to 2 u, the sum of C terms, the division) through sum_i |x_id| dp_ic / S, plus
the penalty term and the final addition -- lr_ref.bound_gradient.  B_f likewise (lr_ref.bound_objective).  Four of them: one for the
device, one for the restatement's own numpy sums, and as much again for what first order leaves out.
dvae_lr_predict, on the device's own coefficients: `counted` and `correct` integer for integer -- a row may differ only where its top
two logits lie within the rounding of the two (2 zeta_i), and the number of such rows is asserted to be 0 on every case --, prob
within 1 fp32 ulp of the restatement's probability rounded once, log_loss within its first-order bound (lr_ref.predict).
Every ratio is printed; DESIGN.md, section 2, records them."""
import functools
import json
import logging
import os

import numpy as np
import pytest
import torch

import lr_ref as R
import predict_ref as P
import sap_ref as SR
from gpu_util import DEV, stream
from guard_util import Guarded, run_contract
from disvae_amd import _lib, _lrlib, Evaluator, explicitness_from_table, infoe_from_log_loss, infoe_from_table
from disvae_amd import evaluate as E

pytestmark = pytest.mark.gpu
TOL = 1e-8
IDS = R.IDS


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype).contiguous()


@functools.lru_cache(maxsize=None)
def case(name):
    c = R.case(name)
    lt = np.ascontiguousarray(c["labels"][:, :c["S"]])
    le = np.ascontiguousarray(c["labels"][:, c["S"]:]).copy()
    le[:, ::7] = -1                                                           # values the training rows do not hold
    assert all(lt[q].min() == 0 and lt[q].max() == C - 1 for q, C in enumerate(c["classes"])) and c["S"] <= _lrlib.MAX_ROWS
    assert c["D"] <= _lrlib.MAX_D and c["Q"] <= _lrlib.MAX_PROBLEMS and max(c["classes"]) <= _lrlib.MAX_CLASSES
    c.update(lt=lt, le=le, sizes=_lrlib.coef_sizes(c["classes"], c["D"]))
    return c


def _shift_scale(c):
    if c["shift"] is None:
        return None, None
    return _dev(c["shift"], torch.float64), _dev(c["scale"], torch.float64)


def run_fit(c, fill=float("nan"), tol=TOL):
    """dvae_lr_fit on poisoned outputs -> (coef, flat; report [Q, 4]) as numpy."""
    S, D, Q = c["S"], c["D"], c["Q"]
    cls = _lrlib.host_classes(c["classes"])
    n_ws = _lrlib.lib().dvae_lr_ws_bytes(S, D, cls, Q)
    assert n_ws > 0 and n_ws % 8 == 0
    xd, ld = _dev(c["X32"][:S], torch.float32), _dev(c["lt"], torch.int32)
    sh, sc = _shift_scale(c)
    ws = torch.full((n_ws // 8,), float("nan"), dtype=torch.float64, device=DEV)
    coef = torch.full((sum(c["sizes"]),), fill, dtype=torch.float64, device=DEV)
    report = torch.full((Q, 4), fill, dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    _lrlib.call("dvae_lr_fit", xd.data_ptr(), None if sh is None else sh.data_ptr(), None if sc is None else sc.data_ptr(), ld.data_ptr(), cls,
                S, D, Q, c["reg_C"], tol, ws.data_ptr(), coef.data_ptr(), report.data_ptr(), stream())
    torch.cuda.synchronize()
    return coef.cpu().numpy(), report.cpu().numpy()


def run_predict(c, coef, X32, labels, with_prob=True):
    T, D, Q = X32.shape[0], c["D"], c["Q"]
    cls = _lrlib.host_classes(c["classes"])
    xd, ld, cd = _dev(X32, torch.float32), _dev(labels, torch.int32), _dev(coef, torch.float64)
    sh, sc = _shift_scale(c)
    prob = torch.full((T * sum(c["classes"]),), float("nan"), dtype=torch.float32, device=DEV) if with_prob else None
    loss = torch.full((Q,), float("nan"), dtype=torch.float64, device=DEV)
    correct = torch.full((Q,), -7, dtype=torch.int32, device=DEV)
    counted = torch.full((Q,), -7, dtype=torch.int32, device=DEV)
    _lrlib.call("dvae_lr_predict", xd.data_ptr(), None if sh is None else sh.data_ptr(), None if sc is None else sc.data_ptr(), ld.data_ptr(), cls,
                T, D, Q, cd.data_ptr(), None if prob is None else prob.data_ptr(), loss.data_ptr(), correct.data_ptr(), counted.data_ptr(), stream())
    torch.cuda.synchronize()
    return (None if prob is None else prob.cpu().numpy()), loss.cpu().numpy(), correct.cpu().numpy(), counted.cpu().numpy()


@functools.lru_cache(maxsize=None)
def device_fit(name):
    return run_fit(case(name))


def thetas(c, coef):
    at = np.concatenate([[0], np.cumsum(c["sizes"])])
    return [coef[at[q]:at[q + 1]] for q in range(c["Q"])]


@functools.lru_cache(maxsize=None)
def host_objectives(name):
    """f at the point fit_logistic_regression reaches (the host's L-BFGS on the same fp64 features), per problem."""
    c = case(name)
    X = c["X"][:c["S"]]
    out = []
    for q, C in enumerate(c["classes"]):
        W, b = E.fit_logistic_regression(torch.from_numpy(X), torch.from_numpy(c["lt"][q].astype(np.int64)), C, C=c["reg_C"])
        out.append(R.objective(X, c["lt"][q], C, c["reg_C"], R.join(W.numpy(), b.numpy())))
    return out


# ---- 1. the fit against the restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", IDS)
def test_fit_meets_the_optimality_conditions(name):
    c = case(name)
    coef, report = device_fit(name)
    S, D = c["S"], c["D"]
    X = c["X"][:S]
    assert np.isfinite(coef).all() and np.isfinite(report).all() and report.shape == (c["Q"], 4)
    for q, (C, theta) in enumerate(zip(c["classes"], thetas(c, coef))):
        y, ref = c["lt"][q], c["problems"][q]
        g = float(np.abs(R.gradient(X, y, C, c["reg_C"], theta)).max())
        B_g, B_f = R.bound_gradient(X, y, C, c["reg_C"], theta), R.bound_objective(X, y, C, c["reg_C"], theta)
        f = R.objective(X, y, C, c["reg_C"], theta)
        norm = R.pinv_norm(R.hessian(X, y, C, c["reg_C"], ref["theta"]), C, D)
        apart = float(np.abs(R.centred(theta, C, D) - ref["theta"]).max())
        allowed = 2.0 * norm * (TOL + 4.0 * B_g)
        f_host = host_objectives(name)[q]
        b = R.split(theta, C, D)[1]
        print("%s[%d]: C = %d, %d steps, %d evaluations; g = %.2e (tolerance + %.3g B_g, B_g = %.1e); report's g off by %.3g B_g; "
              "|theta - theta*| = %.2e (allowed %.2e, ||H+|| = %.1e); f - f_host = %.2e (B_f = %.1e), report's f off by %.3g B_f; sum b = %.1e"
              % (name, q, C, report[q, 2], report[q, 3], g, max(g - TOL, 0.0) / B_g, B_g, abs(report[q, 1] - g) / B_g, apart, allowed, norm,
                 f - f_host, B_f, abs(report[q, 0] - f) / B_f, b.sum()))
        assert 0 <= report[q, 2] <= _lrlib.MAX_ITERATIONS // 4 and report[q, 2] == int(report[q, 2])      # converged, far from the bound
        assert report[q, 2] + 1 <= report[q, 3] <= report[q, 2] * (_lrlib.MAX_HALVINGS + 1) + 1
        assert ref["gmax"] <= 1e-13 and ref["iterations"] >= 0
        assert g <= TOL + 4.0 * B_g, (name, q, g)
        assert abs(report[q, 1] - g) <= 4.0 * B_g, (name, q, report[q, 1], g)
        assert apart <= allowed, (name, q, apart, allowed)
        assert f <= f_host + 4.0 * B_f, (name, q, f, f_host)
        assert abs(report[q, 0] - f) <= 4.0 * B_f, (name, q, report[q, 0], f)
        assert abs(b.sum()) <= 1e-10 * max(1.0, float(np.abs(b).max()))       # the solver stays on sum b = 0, to rounding
        if name.startswith("constant"):
            assert (R.split(theta, C, D)[0][:, -1] == 0.0).all()              # exactly 0, not merely small
            assert np.abs(R.split(theta, C, D)[0][:, :-1]).min() > 0.0


@pytest.mark.parametrize("name", IDS)
def test_predict_on_the_devices_own_coefficients(name):
    c = case(name)
    coef, _report = device_fit(name)
    S = c["S"]
    for X32, X, labels in ((c["X32"][:S], c["X"][:S], c["lt"]), (c["X32"][S:], c["X"][S:], c["le"])):
        prob, loss, correct, counted = run_predict(c, coef, X32, labels)
        only, loss2, correct2, counted2 = run_predict(c, coef, X32, labels, with_prob=False)
        assert only is None and loss2.tobytes() == loss.tobytes() and np.array_equal(correct, correct2) and np.array_equal(counted, counted2)
        at = 0
        for q, (C, theta) in enumerate(zip(c["classes"], thetas(c, coef))):
            want = R.predict(X, labels[q], theta, C)
            near_ties = int((want["gap"] <= 2.0 * want["dz"]).sum()) if C >= 2 else 0
            got = prob[at:at + len(X) * C].reshape(len(X), C)
            at += len(X) * C
            want32 = want["prob"].astype(np.float32)
            ulps = np.abs(got.astype(np.float64) - want32.astype(np.float64)) / np.spacing(np.maximum(want32, np.float32(1e-45))).astype(np.float64)
            ratio = abs(loss[q] - want["log_loss"]) / want["bound"] if want["bound"] > 0 else 0.0
            print("%s[%d] %d rows: counted %d, correct %d, %d near-ties, prob at most %.2f fp32 ulp off, log_loss off by %.3f of its bound"
                  % (name, q, len(X), counted[q], correct[q], near_ties, ulps.max(), ratio))
            assert near_ties == 0
            assert counted[q] == want["counted"] == int((labels[q] >= 0).sum())
            assert correct[q] == want["correct"]
            assert ulps.max() <= 1.0
            assert abs(loss[q] - want["log_loss"]) <= want["bound"]
    assert (c["le"] == -1).any()


def test_ties_go_to_the_lowest_class():
    c = dict(case("rows-63"))
    coef = np.zeros(sum(c["sizes"]))                                          # every logit 0: class 0 everywhere, every probability 1 / C
    S = c["S"]
    prob, loss, correct, counted = run_predict(c, coef, c["X32"][:S], c["lt"])
    assert np.array_equal(correct, [(c["lt"][q] == 0).sum() for q in range(c["Q"])]) and np.array_equal(counted, [S, S])
    assert (prob[:2 * S] == np.float32(0.5)).all() and (prob[2 * S:] == np.float32(1.0 / 3.0)).all()
    assert loss[0] == pytest.approx(S * np.log(2.0), rel=1e-14) and loss[1] == pytest.approx(S * np.log(3.0), rel=1e-14)


# ---- 2. determinism, memory ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rows-2", "rows-65-five-problems", "rows-512-256-classes", "max-rows", "d17", "offset-scaled"])
def test_same_bits_twice_with_poisoned_outputs(name):
    a, ra = device_fit(name)
    b, rb = run_fit(case(name), fill=-1e300)
    assert a.tobytes() == b.tobytes() and ra.tobytes() == rb.tobytes()


def _call(name):
    return lambda args: _lrlib.call(name, *[a.ptr if isinstance(a, Guarded) else a for a in args])


@pytest.mark.parametrize("name", ["rows-2", "rows-65-five-problems", "rows-513-one-row-class", "d17", "offset-scaled", "rows-512-256-classes"])
def test_memory_contract(name):
    """Guards untouched, inputs unchanged, every output element written, bits equal to the run on plain tensors whatever the
    surroundings hold (NaN at 256-byte alignment; -1e30 at the weakest alignment promised: the element's own) -- dvae_lr_fit,
    dvae_lr_predict with and without prob."""
    c = case(name)
    S, T, D, Q = c["S"], c["T"], c["D"], c["Q"]
    cls = _lrlib.host_classes(c["classes"])
    n_ws = _lrlib.lib().dvae_lr_ws_bytes(S, D, cls, Q) // 8
    coef, report = device_fit(name)

    def scaling(al):
        if c["shift"] is None:
            return [None, None]
        return [al.inp("shift", torch.from_numpy(c["shift"]), align=8, dtype=torch.float64),
                al.inp("scale", torch.from_numpy(c["scale"]), align=8, dtype=torch.float64)]

    def build_fit(al):
        return [al.inp("features", c["X32"][:S], align=4)] + scaling(al) + [
            al.inp("labels", torch.from_numpy(c["lt"]), align=4), cls, S, D, Q, c["reg_C"], TOL, al.ws("ws", (n_ws,), dtype=torch.float64, align=8),
            al.out("coef", (len(coef),), dtype=torch.float64, align=8), al.out("report", (Q, 4), dtype=torch.float64, align=8), stream()]
    runs = run_contract("dvae_lr_fit", build_fit, fn=_call("dvae_lr_fit"))
    by_name = {g.name: g for g in runs[0].args}
    assert by_name["coef"].t.cpu().numpy().tobytes() == coef.tobytes() and by_name["report"].t.cpu().numpy().tobytes() == report.tobytes()

    for with_prob in (True, False):
        def build_predict(al):
            return [al.inp("features", c["X32"][S:], align=4)] + scaling(al) + [
                al.inp("labels", torch.from_numpy(c["le"]), align=4), cls, T, D, Q, al.inp("coef", torch.from_numpy(coef), align=8, dtype=torch.float64),
                al.out("prob", (T * sum(c["classes"]),), dtype=torch.float32, align=4) if with_prob else None,
                al.out("log_loss", (Q,), dtype=torch.float64, align=8), al.out("correct", (Q,), dtype=torch.int32, align=4),
                al.out("counted", (Q,), dtype=torch.int32, align=4), stream()]
        runs = run_contract("dvae_lr_predict", build_predict, fn=_call("dvae_lr_predict"))
        by_name = {g.name: g for g in runs[0].args}
        prob, loss, correct, counted = run_predict(c, coef, c["X32"][S:], c["le"], with_prob=with_prob)
        assert by_name["log_loss"].t.cpu().numpy().tobytes() == loss.tobytes()
        assert np.array_equal(by_name["correct"].t.cpu().numpy(), correct) and np.array_equal(by_name["counted"].t.cpu().numpy(), counted)
        if with_prob:
            assert by_name["prob"].t.cpu().numpy().tobytes() == prob.tobytes()


def test_a_problem_that_cannot_meet_the_tolerance_reports_minus_one():
    """tolerance_grad = 0 is below the rounding of the gradient: the solve ends at the bound or without an acceptable step, says so in
    the report, and still returns the point it reached (finite, every element written)."""
    c = case("rows-63")
    coef, report = run_fit(c, tol=0.0)
    assert np.isfinite(coef).all() and (report[:, 2] == -1).all() and (report[:, 1] < 1e-12).all() and (report[:, 3] >= 2).all()
    with pytest.raises(_lib.DvaeHipError, match=r"problem 0 .*did not meet tolerance_grad"):
        E.fit_logistic_regression_device(_dev(c["X32"][:c["S"]], torch.float32), _dev(c["lt"][0], torch.int64), 2, tolerance_grad=0.0)


# ---- 3. end to end ------------------------------------------------------------------------------------------------------------------
def _entangled_rows():
    """The selection of test_gpu_prediction_scores on the N = 60 entangled table: no training row with factor 1 = 3, no test row with
    factor 2 = 4."""
    factors = P.factor_table(P.SMALL)
    order = np.random.default_rng(9).permutation(60)
    train = [r for r in order if factors[r, 1] != 3][:40]
    rest = [r for r in order if r not in train and factors[r, 2] != 4]
    test = sorted(rest, key=lambda r: factors[r, 1] == 3)[:12]
    return np.array(train + test)


FIXTURES = {"ideal-960": (P.LARGE, lambda: P.ideal_table(P.LARGE), lambda: P.drawn_rows(960, 960, 1), 600, 360),
            "entangled-60": (P.SMALL, lambda: P.entangled_table(P.SMALL), _entangled_rows, 40, 12)}


@pytest.mark.parametrize("name", list(FIXTURES))
def test_explicitness_with_the_device_fit_against_the_host_fit(name):
    """Within 2.8e-5: what test_prediction_scores_host.py grants two converged optimisers."""
    sizes, tab, rows, n_train, n_test = FIXTURES[name]
    table, rows = _dev(tab(), torch.float32), rows()
    host, host_details = explicitness_from_table(table, sizes, n_train=n_train, n_test=n_test, rows=rows, return_details=True)
    dev, dev_details = explicitness_from_table(table, sizes, n_train=n_train, n_test=n_test, rows=rows, return_details=True, fit="device")
    assert set(host) == set(dev)
    worst = 0.0
    for key in host:
        a, b = np.asarray(host[key], dtype=np.float64), np.asarray(dev[key], dtype=np.float64)
        assert np.array_equal(np.isnan(a), np.isnan(b)), key
        if a.size and (~np.isnan(a)).any():
            worst = max(worst, float(np.nanmax(np.abs(a - b))))
    apart = max(float((R.centred(R.join(h["W"].numpy(), h["b"].numpy()), len(h["b"]), 6)
                       - R.centred(R.join(d["W"].numpy(), d["b"].numpy()), len(d["b"]), 6)).__abs__().max()) for h, d in zip(host_details, dev_details))
    print("%s: explicitness host %.9f / %.9f, device %.9f / %.9f: at most %.2e apart (allowed 2.8e-5); coefficients at most %.2e apart"
          % (name, host["explicitness_train"], host["explicitness_test"], dev["explicitness_train"], dev["explicitness_test"], worst, apart))
    assert worst <= 2.8e-5
    for h, d in zip(host_details, dev_details):
        assert d["probabilities_train"].dtype == torch.float32 and d["probabilities_train"].shape == h["probabilities_train"].shape
        assert torch.equal(d["labels_test"], h["labels_test"]) and torch.equal(d["classes"], h["classes"])


@pytest.mark.parametrize("name", list(FIXTURES))
def test_beta_vae_accuracies_with_the_device_fit_equal_the_host_fit(name):
    """Equal, but for rows whose top two logits (the host's) lie within what the coefficient difference of the two fits can move them:
    2 delta (||x||_1 + 1); their number is asserted to be 0."""
    sizes, tab, _rows, _n_train, _n_test = FIXTURES[name]
    table = _dev(tab(), torch.float32)
    kw = dict(n_train=300, n_eval=150, batch_size=8, n_variance=60, seed=5)
    host, hd = E.factor_scores_from_table(table, sizes, return_details=True, **kw)
    dev, dd = E.factor_scores_from_table(table, sizes, return_details=True, fit="device", **kw)
    C = len(hd["classes"])
    delta = float(np.abs(R.centred(R.join(hd["W"].numpy(), hd["b"].numpy()), C, 6) - R.centred(R.join(dd["W"].numpy(), dd["b"].numpy()), C, 6)).max())
    near = 0
    for key in ("train", "eval"):
        x = hd["features_" + key].numpy()
        z = np.sort(x @ hd["W"].numpy().T + hd["b"].numpy(), axis=1)
        near += int((z[:, -1] - z[:, -2] <= 2.0 * delta * (np.abs(x).sum(axis=1) + 1.0)).sum())
        assert torch.equal(hd["features_" + key], dd["features_" + key]) and torch.equal(hd["labels_" + key], dd["labels_" + key])
    print("%s: beta-VAE host %.4f / %.4f, device %.4f / %.4f; coefficients %.2e apart, %d near-ties"
          % (name, host["beta_vae_train"], host["beta_vae_eval"], dev["beta_vae_train"], dev["beta_vae_eval"], delta, near))
    assert near == 0 and set(host) == set(dev)
    assert all(host[k] == dev[k] for k in host), (host, dev)


@functools.lru_cache(maxsize=None)
def _infoe_tables():
    rows = SR.end_to_end_rows()
    states = torch.get_rng_state(), torch.cuda.get_rng_state()
    got = {name: infoe_from_table(_dev(tab, torch.float32), SR.GRID, n_train=240, n_test=120, rows=rows) for name, tab in SR.end_to_end_tables().items()}
    unchanged = torch.equal(states[0], torch.get_rng_state()) and torch.equal(states[1], torch.cuda.get_rng_state())
    return got, unchanged


INFOE_KEYS = {"infoe_train", "infoe_test", "infoe_train_per_factor", "infoe_test_per_factor", "ce_model_train", "ce_model_test", "ce_null_train",
              "ce_null_test", "accuracy_train", "accuracy_test", "n_unseen", "report", "n_train", "n_test", "C", "standardize"}


def test_infoe_against_the_restatement_and_its_order():
    """InfoE of the device's fits against infoe_reference (the reference optimum).  A cross-entropy moves by at most 2 max |d logit| <=
    2 (max_i ||x_i||_1 + 1) ||d theta||_inf, and ||d theta||_inf <= 2 ||H^+||_inf (1e-8 + 4 B_g): the bound of every factor, divided by
    ce_null for InfoE.  infoe_train >= -1e-12 on every factor: theta = (0, log frequencies) is feasible at no penalty.
    The order ideal > rotated > independent of the factors: a linear probe on ALL latents does not see a rotation, so the first gap
    is small (2.8e-3 on the restatement, test_lr_host.py) -- it comes from the standardisation of the mixed columns and the penalty --
    and is still 1e3 times the bound above."""
    got, unchanged = _infoe_tables()
    rows = SR.end_to_end_rows()
    assert unchanged
    for name, tab in SR.end_to_end_tables().items():
        g = got[name]
        ref = R.infoe_reference(tab, SR.GRID, rows[:240], rows[240:])
        assert set(g) == INFOE_KEYS and g["report"].shape == (4, 4) and (g["report"][:, 2] >= 0).all()
        Xt = R.features(tab[rows[:240]], ref["shift"], ref["scale"])
        lt, _le, n = R.rank_labels(rows[:240], rows[240:], SR.GRID)
        worst = 0.0
        for k, C in enumerate(n):
            theta = ref["thetas"][k]
            move = 2.0 * R.pinv_norm(R.hessian(Xt, lt[k], C, 1.0, theta), C, 6) * (TOL + 4.0 * R.bound_gradient(Xt, lt[k], C, 1.0, theta))
            for key, X in (("train", Xt), ("test", R.features(tab[rows[240:]], ref["shift"], ref["scale"]))):
                bound = 2.0 * (np.abs(X).sum(axis=1).max() + 1.0) * move + 1e-12
                err = abs(g["ce_model_" + key][k] - ref["ce_model_" + key][k])
                worst = max(worst, err / bound)
                assert err <= bound, (name, k, key, err, bound)
                assert abs(g["ce_null_" + key][k] - ref["ce_null_" + key][k]) <= 1e-13
                assert abs(g["infoe_%s_per_factor" % key][k] - ref["infoe_%s_per_factor" % key][k]) <= bound / ref["ce_null_" + key][k] + 1e-12
                assert g["accuracy_" + key][k] == ref["accuracy_" + key][k]
        assert (g["infoe_train_per_factor"] >= -1e-12).all() and (g["n_unseen"] == 0).all()
        assert g["infoe_train"] == float(np.maximum(g["infoe_train_per_factor"], 0.0).mean())
        assert g["infoe_train"] == infoe_from_log_loss(g["ce_model_train"], g["ce_null_train"])[1]
        print("%s: InfoE %.6f / %.6f (restatement %.6f / %.6f), cross-entropies within %.3f of their bound, at most %d Newton steps, %d evaluations"
              % (name, g["infoe_train"], g["infoe_test"], ref["infoe_train"], ref["infoe_test"], worst, g["report"][:, 2].max(), g["report"][:, 3].max()))
    assert got["ideal"]["infoe_train"] > got["rotated"]["infoe_train"] > got["collapsed"]["infoe_train"]
    assert got["ideal"]["infoe_test"] > got["rotated"]["infoe_test"] > got["collapsed"]["infoe_test"]


def test_infoe_seed_unseen_values_and_one_class():
    td = _dev(SR.end_to_end_tables()["ideal"], torch.float32)
    cpu0, dev0 = torch.get_rng_state(), torch.cuda.get_rng_state()
    a = infoe_from_table(td, SR.GRID, n_train=200, n_test=100, seed=3)
    b = infoe_from_table(td, SR.GRID, n_train=200, n_test=100, seed=3)
    other = infoe_from_table(td, SR.GRID, n_train=200, n_test=100, seed=4)
    assert torch.equal(torch.get_rng_state(), cpu0) and torch.equal(torch.cuda.get_rng_state(), dev0)
    assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)
    assert a["report"].tobytes() != other["report"].tobytes()
    same = np.random.default_rng(6).permutation(120)                         # rows 0 .. 119: factor 0 takes the value 0 only
    flat = infoe_from_table(td, SR.GRID, n_train=80, n_test=40, rows=same)
    assert np.isnan(flat["infoe_train_per_factor"][0]) and np.isnan(flat["infoe_test_per_factor"][0]) and flat["accuracy_test"][0] == 1.0
    assert flat["infoe_train"] == float(np.maximum(flat["infoe_train_per_factor"][1:], 0.0).mean())
    raw = infoe_from_table(td, SR.GRID, n_train=200, n_test=100, seed=3, standardize=False, C=10.0)
    assert raw["standardize"] is False and raw["C"] == 10.0 and raw["infoe_train"] > a["infoe_train"]       # a weaker penalty fits closer
    with pytest.raises(ValueError, match="NaN or an infinity"):
        bad = td.clone()
        bad[7, 2] = float("inf")
        infoe_from_table(bad, SR.GRID, n_train=240, n_test=120)


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
    lat_sizes, lat_names = np.array(SR.GRID), tuple("abcd")

    def __len__(self):
        return 360


class _Loader:
    dataset = _Factors()

    def __iter__(self):
        for lo in range(0, 360, 100):
            yield torch.arange(lo, min(lo + 100, 360), dtype=torch.float32).view(-1, 1), None


def test_evaluator_end_to_end(tmp_path):
    tab = SR.end_to_end_tables()["ideal"]
    model = _TableModel(tab).train()
    ev = Evaluator(model, None, device=torch.device(DEV), logger=logging.getLogger("lr"), save_dir=str(tmp_path), is_progress_bar=False)
    kw = dict(n_train=240, n_test=120, seed=2)
    got = ev.compute_infoe(_Loader(), **kw)
    assert model.training and model.modes == [False] * 4                     # encoded in eval mode, mode restored
    direct = infoe_from_table(_dev(tab, torch.float32), SR.GRID, **kw)
    assert all(np.asarray(got[k]).tobytes() == np.asarray(direct[k]).tobytes() for k in got) and got["infoe_train"] > 0.5
    e_host = ev.compute_explicitness(_Loader(), **kw)
    e_dev = ev.compute_explicitness(_Loader(), fit="device", **kw)
    assert abs(e_host["explicitness_test"] - e_dev["explicitness_test"]) <= 2.8e-5
    s_dev = ev.compute_factor_scores(_Loader(), n_train=100, n_eval=50, batch_size=8, n_variance=100, fit="device")
    assert 0.0 <= s_dev["beta_vae_eval"] <= 1.0
    assert ev(_Loader(), is_losses=False) == (None, None) and os.listdir(tmp_path) == []
    assert ev(_Loader(), is_losses=False, is_infoe=True, infoe_args=kw) == (None, None)
    assert os.listdir(tmp_path) == ["infoe.log"]                             # and nothing else new
    logged = json.load(open(tmp_path / "infoe.log"))
    assert set(logged) == set(got) - {"report"}
    assert logged["infoe_train"] == got["infoe_train"] and logged["infoe_test_per_factor"] == got["infoe_test_per_factor"].tolist()
    with pytest.raises(ValueError, match=r"n_train \+ n_test must be at most 360"):
        ev.compute_infoe(_Loader())                                          # the defaults want 15 000 rows
