"""-m gpu: the semi-supervised S2-beta-VAE loss -- libdvae_semi_hip.so through its C-ABI against the fp64 restatement
(tests/semi_ref.py), and whole training steps of SemiSupervisedVaeLoss against the oracle.

Kernel level.  n in {1, 2} and one row on either side of DVAE_SEMI_BLOCK_ROWS (one workgroup / two), two chunks + 1 and the limit
16 384; D in {1, 10, 16, 17, 64} (and 5, 8 for K = D); K in {1, 3, 5, 8}; the five labelling patterns; dSprites' sizes, a table
with a size-1 factor, one factor, eight factors; split and interleaved means; both reductions; the five tables of semi_ref.
n_lab is exact and dmu is an exact zero wherever it is defined as zero; values and C are inside the fp64 accumulation bounds of
semi_ref; gradients are inside semi_ref.tol_dmu, whose fp32 part carries the margin max(1, 4 e32) = 4.24 (e32 = 1.06:
semi_ref.E32_WORST, measured on the CPU and pinned by tests/test_semi_host.py).  Every case prints the worst error / bound at
margin 1 before it asserts.

Whole step, shaped like test_gpu_dip.py::test_fused_step_vs_oracle, same tolerances: loss 2e-5; gradients rtol 1e-5 + 2e-6
max|g| against the gate-matched fp64 oracle at the engine's parameters, three steps, no outliers.
"""
import ctypes
import functools
from collections import defaultdict

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import semi_ref as R
from gpu_util import DEV, check, dev, stream
from guard_util import Guarded, run_contract
from oracle import disvae_oracle as O
from oracle.gate_match import engine_gates, gate_mismatches
from disvae_amd import _lib, _semilib
from disvae_amd.data import LabelledFactorLoader
from disvae_amd.evaluate import Evaluator
from disvae_amd.models.losses import get_loss_f
from disvae_amd.models.vae import init_specific_model
from disvae_amd.training import Trainer
from test_gpu_step_poison import _poison

CH = _semilib.BLOCK_ROWS
EIGHT = (2, 3, 2, 4, 3, 2, 5, 2)
SIZES = {"dsprites": R.DSPRITES, "one_value": R.ONE_VALUE, "one_factor": (1, 7, 1), "eight": EIGHT}     # K = 5, 3, 1, 8
W = 0.75
# (n, D, sizes, pattern, reduction, interleaved)
CASES = [(1, 1, "one_factor", "all", "sum", 0), (1, 10, "dsprites", "none", "mean", 0), (2, 10, "dsprites", "all", "mean", 1),
         (2, 16, "eight", "alternating", "sum", 0), (CH - 1, 17, "dsprites", "second_half", "sum", 1),
         (CH, 10, "dsprites", "alternating", "mean", 0), (CH, 8, "eight", "all", "sum", 0), (CH + 1, 10, "dsprites", "last", "sum", 0),
         (CH + 1, 64, "eight", "second_half", "mean", 1), (2 * CH + 1, 10, "one_value", "alternating", "sum", 0),
         (2 * CH + 1, 16, "dsprites", "none", "sum", 0), (2 * CH + 1, 5, "dsprites", "all", "mean", 0),
         (2 * CH + 1, 1, "one_factor", "second_half", "sum", 0), (_semilib.MAX_ROWS, 10, "dsprites", "alternating", "mean", 0),
         (_semilib.MAX_ROWS, 64, "eight", "last", "sum", 1), (_semilib.MAX_ROWS, 17, "one_value", "all", "sum", 0)]


@functools.lru_cache(maxsize=None)
def _reference(kind, table, n, D, sizes, pattern, reduction):
    """(mu, rows, restatement): computed once, shared by the tests, never written to."""
    mu, rows = R.table(table, n, D), R.rows_for(n, SIZES[sizes], pattern)
    return mu, rows, R.regulariser(mu, rows, SIZES[sizes], kind, reduction, w=W)


def _launch(mu, rows, sizes, kind, reduction, interleaved=0, grads=True, loss0=None, w=W):
    """The two launches on device copies -> (out fp64 [2 + D K], dmu, loss_io) as numpy."""
    n, D = mu.shape
    factors = R.default_factors(sizes)
    K = len(factors)
    tab = _semilib.factor_table(sizes, factors)
    if interleaved:
        ml = np.full((n, 2 * D), np.nan, np.float32)                      # the log-variance half is never read
        ml[:, 0::2] = mu
        mu_t = torch.tensor(ml, device=DEV)
    else:
        mu_t = torch.tensor(mu, device=DEV)
    rows_t = torch.tensor(rows, device=DEV)
    ws = torch.full((_semilib.ws_doubles(n, D, K),), float("nan"), dtype=torch.float64, device=DEV)
    out = torch.full((_semilib.out_doubles(D, K),), float("nan"), dtype=torch.float64, device=DEV)
    g = torch.full((n, D), float("nan"), device=DEV) if grads else None
    w_t = torch.tensor([w], dtype=torch.float32, device=DEV)
    lio = None if loss0 is None else torch.tensor([loss0], dtype=torch.float32, device=DEV)
    p = lambda t: None if t is None else t.data_ptr()
    ps, pt = ctypes.addressof(tab[0]), ctypes.addressof(tab[1])
    k, r = _semilib.KINDS[kind], _semilib.REDUCTIONS[reduction]
    _semilib.call("dvae_semi_partials", p(mu_t), interleaved, p(rows_t), n, D, K, ps, pt, k, p(ws), stream())
    _semilib.call("dvae_semi_grad", p(mu_t), interleaved, p(rows_t), n, D, K, ps, pt, k, r, p(w_t), p(ws), p(g), p(out), p(lio), stream())
    torch.cuda.synchronize()
    c = lambda t: None if t is None else t.cpu().numpy()
    return c(out), c(g), c(lio)


@pytest.mark.parametrize("table", R.TABLES)
@pytest.mark.parametrize("kind", R.KINDS)
def test_kernels_against_the_restatement(kind, table):
    worst = dict(R=0.0, C=0.0, dmu=0.0)
    for n, D, sizes, pattern, reduction, il in CASES:
        mu, rows, ref = _reference(kind, table, n, D, sizes, pattern, reduction)
        out, g, lio = _launch(mu, rows, SIZES[sizes], kind, reduction, il, loss0=3.25)
        K = ref["K"]
        what = "%s %s n=%d D=%d %s %s %s il=%d" % (kind, table, n, D, sizes, pattern, reduction, il)
        assert np.isfinite(out).all() and np.isfinite(g).all(), what
        assert out[1] == ref["n_lab"], what + ": n_lab"                               # integer for integer
        assert not g[R.defined_zero(ref)].any(), what + ": dmu is not zero where it is defined as zero"
        C = out[2:].reshape(D, K)
        tol1, tol = R.tol_dmu(ref), R.tol_dmu(ref, R.MARGIN)
        ratios = dict(R=abs(out[0] - ref["R"]) / (ref["tol_R"] + 1e-300), C=(np.abs(C - ref["C"]) / (ref["tol_C"] + 1e-300)).max(),
                      dmu=(np.abs(g - ref["dmu"]) / tol1).max())
        for k_, v_ in ratios.items():
            worst[k_] = max(worst[k_], float(v_))
        assert abs(out[0] - ref["R"]) <= ref["tol_R"], what + ": R %.17g vs %.17g" % (out[0], ref["R"])
        assert (np.abs(C - ref["C"]) <= ref["tol_C"]).all(), what + ": C"             # (xent / l2, n_lab <= 1: the bound is zero, and so is C)
        assert (np.abs(g - ref["dmu"]) <= tol).all(), what + ": dmu %.3g x the bound at margin 1" % ratios["dmu"]
        if kind == "xent":                                                            # |sigmoid - y| <= 1, also at +-100
            assert np.abs(g).max() <= W * ref["scale"] * (1 + 2.0 ** -23), what
        if ref["n_lab"] == 0:
            assert out[0] == 0.0 and not g.any() and not C.any(), what
        # loss_io is changed by exactly + w R (one fp32 add of the rounded product)
        assert lio[0] == np.float32(3.25) + np.float32(np.float64(np.float32(W)) * out[0]), what
    print("%s %s: worst error / bound -- R %.3g, C %.3g, dmu %.3g at margin 1 (allowed: %g)"
          % (kind, table, worst["R"], worst["C"], worst["dmu"], R.MARGIN))


@pytest.mark.parametrize("kind", R.KINDS)
def test_two_runs_and_the_value_only_launch_give_the_same_bits(kind):
    for n, D, sizes, pattern, reduction, il in (CASES[4], CASES[8], CASES[9], CASES[14]):
        mu, rows, ref = _reference(kind, "regime", n, D, sizes, pattern, reduction)
        a = _launch(mu, rows, SIZES[sizes], kind, reduction, il, loss0=-1.5)
        b = _launch(mu, rows, SIZES[sizes], kind, reduction, il, loss0=-1.5)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes(), (kind, n, D)
        value_only = _launch(mu, rows, SIZES[sizes], kind, reduction, il, grads=False)
        assert value_only[0].tobytes() == a[0].tobytes() and value_only[1] is None and value_only[2] is None
        # the weight scales the gradient and the loss, not `out`
        c = _launch(mu, rows, SIZES[sizes], kind, reduction, il, loss0=-1.5, w=0.0)
        assert c[0].tobytes() == a[0].tobytes() and not c[1].any() and c[2][0] == np.float32(-1.5)


def test_sizes_above_the_limits_are_refused():
    t = torch.zeros(8 * 130, device=DEV)
    rows = torch.zeros(8, dtype=torch.int64, device=DEV)
    w = torch.zeros(1 << 12, dtype=torch.float64, device=DEV)
    tab = _semilib.factor_table((2,) * 9, list(range(9)))
    ps, pt = ctypes.addressof(tab[0]), ctypes.addressof(tab[1])
    for n, D, K, macro in ((8, 65, 5, "DVAE_SEMI_MAX_D"), (8, 10, 9, "DVAE_SEMI_MAX_K"), (16385, 10, 5, "DVAE_SEMI_MAX_ROWS")):
        for name, args in (("dvae_semi_partials", (t.data_ptr(), 0, rows.data_ptr(), n, D, K, ps, pt, 0, w.data_ptr(), stream())),
                           ("dvae_semi_grad", (t.data_ptr(), 0, rows.data_ptr(), n, D, K, ps, pt, 0, 0, t.data_ptr(), w.data_ptr(), None,
                                               w.data_ptr(), None, stream()))):
            with pytest.raises(_lib.DvaeHipError, match="invalid argument.*" + macro):
                _semilib.call(name, *args)
        assert _semilib.lib().dvae_semi_ws_doubles(n, D, K) == 0
    torch.cuda.synchronize()
    assert not t.any() and not w.any()


def _semi_call(name):
    return lambda args: _semilib.call(name, *[a.ptr if isinstance(a, Guarded) else a for a in args])


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("case", [CASES[2], CASES[4], CASES[8], CASES[9]], ids=lambda c: "n%d-D%d-%s-%s" % c[:4])
def test_memory_contract(case, kind):
    """Guard-banded, NaN-poisoned buffers at 256-byte alignment and at the weakest the header promises (4 bytes for the fp32
    arguments, 8 for rows, ws and out): guards untouched, inputs unchanged, every defined output written, the same bits in all
    runs."""
    n, D, sizes, pattern, reduction, il = case
    mu, rows, ref = _reference(kind, "gauss", n, D, sizes, pattern, reduction)
    K = ref["K"]
    tab = _semilib.factor_table(SIZES[sizes], R.default_factors(SIZES[sizes]))
    ps, pt = ctypes.addressof(tab[0]), ctypes.addressof(tab[1])
    k, r = _semilib.KINDS[kind], _semilib.REDUCTIONS[reduction]
    if il:
        ml = np.zeros((n, 2 * D), np.float32)
        ml[:, 0::2] = mu
    else:
        ml = mu
    groups, rd = _semilib.groups(n), _semilib.rec_doubles(D, K)
    rec = np.zeros((groups, rd), dtype=bool)
    rec[:, :2] = True
    rec[:, 2:] = kind == "cov"
    defined = torch.tensor(rec.reshape(-1))

    def partials(al):
        return [al.inp("mu", ml, align=4), il, al.inp("rows", rows, align=8), n, D, K, ps, pt, k,
                al.out("ws", (groups * rd,), dtype=torch.float64, align=8, written=defined), stream()]
    runs = run_contract("dvae_semi_partials", partials, fn=_semi_call("dvae_semi_partials"))
    ws = runs[0].args[-1].t.clone()
    ws[~defined.to(ws.device)] = float("nan")                             # what the first launch leaves undefined is never read

    def grad(al):
        return [al.inp("mu", ml, align=4), il, al.inp("rows", rows, align=8), n, D, K, ps, pt, k, r,
                al.inp("w", torch.tensor([W]), align=4), al.inp("ws", ws, align=8, dtype=torch.float64), al.out("dmu", (n, D), align=4),
                al.out("out", (2 + D * K,), dtype=torch.float64, align=8), al.inout("loss_io", torch.tensor([2.5]), align=4), stream()]
    runs = run_contract("dvae_semi_grad", grad, fn=_semi_call("dvae_semi_grad"))
    got = {g.name: g.t.cpu().numpy() for g in runs[2].args}
    assert (np.abs(got["dmu"] - ref["dmu"]) <= R.tol_dmu(ref, R.MARGIN)).all() and got["out"][1] == ref["n_lab"]
    assert got["loss_io"][0] == np.float32(2.5) + np.float32(np.float64(np.float32(W)) * got["out"][0])

    def value_only(al):
        a = grad(al)
        al.args[:] = [g for g in al.args if g.name not in ("dmu", "loss_io")]
        return a[:12] + [None, a[13], None, a[15]]
    runs = run_contract("dvae_semi_grad (value only)", value_only, fn=_semi_call("dvae_semi_grad"))
    assert runs[2].args[-1].t.cpu().numpy().tobytes() == got["out"].tobytes()


# ---- whole steps ------------------------------------------------------------------------------------------------------------------
HP = dict(rec_dist="bernoulli", reg_anneal=10000, betaH_B=4, betaB_initC=0, betaB_finC=25, betaB_G=1000, factor_G=6.4,
          lr_disc=1e-4, btcvae_A=1, btcvae_B=6.4, btcvae_G=1, n_data=737280, lat_sizes=R.DSPRITES, s2_beta=4)
GAMMA = {"xent": 4.0, "l2": 4.0, "cov": 0.015625}                          # exact in fp32: the device reads w_t as a float
G_RTOL, G_ATOL = 1e-5, 2e-6
STEP_CASES = [(kind, img, B, D, dist) for kind in R.KINDS
              for img, B, D, dist in (((1, 32, 32), 16, 10, "bernoulli"), ((3, 64, 64), 12, 20, "gaussian"))]


def _native(hp, img, D, seed, lr, loss="s2vae"):
    torch.manual_seed(seed)
    model = init_specific_model("Burgess", img, D)
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    loss_f = get_loss_f(loss, device=torch.device(DEV), latent_dim=D, **hp)
    model.to(DEV)
    model.train()
    return model, opt, loss_f


def _rows(B, step, pattern="second_half"):
    return R.rows_for(B, R.DSPRITES, pattern, seed=step)


@pytest.mark.parametrize("kind,img,B,D,rec_dist", STEP_CASES)
def test_fused_step_vs_oracle(kind, img, B, D, rec_dist):
    seed, lr = 1234, 5e-4
    hp = dict(HP, rec_dist=rec_dist, sup_loss=kind, gamma_sup=GAMMA[kind], latent_dim=D)
    model, opt, loss_f = _native({k: v for k, v in hp.items() if k != "latent_dim"}, img, D, seed, lr)
    gen = torch.Generator().manual_seed(seed + 1)
    for step in range(3):
        data = torch.rand((B,) + tuple(img), generator=gen)
        eps = torch.randn(B, D, generator=gen)
        rows = _rows(B, step, ("second_half", "alternating", "last")[step])
        p_step = {k: p.detach().cpu().clone() for k, p in model.named_parameters()}
        st = O.LossState(rec_dist=rec_dist, steps_anneal=HP["reg_anneal"]); st.n_train_steps = step
        ref_loss, ref_logs, _, ref_outs = R.semi_iteration_grads(hp, st, O.clone_params(p_step, requires_grad=True), data, eps, rows)
        storer = defaultdict(list)
        out = loss_f.fused_step(dev(data), model, opt, storer, eps=dev(eps), labels=torch.tensor(rows, device=DEV))
        buf = model.engine.buffers(B)
        print("%s step %d: loss %.6f (oracle %.6f), sup %.6f" % (kind, step, out.item(), ref_loss.item(), ref_logs["sup_loss"].item()))
        np.testing.assert_allclose(out.item(), ref_loss.item(), rtol=2e-5, err_msg="loss step %d" % step)
        check(buf.mu, ref_outs["mu"], what="mu")
        check(buf.logvar, ref_outs["logvar"], what="logvar")
        check(buf.recon, ref_outs["recon"], what="recon")
        gates = engine_gates(model, B)
        log = []
        with torch.no_grad(), O.gates(None, record=log):
            O.vae_forward(O.clone_params(p_step, dtype=torch.float64), data.double(), eps.double())
        n_diff, gate_worst, ok = gate_mismatches(gates, log)
        assert ok, "a ReLU gated differently than in fp64 at |pre-activation| = %.2e of the layer scale" % gate_worst
        st64 = O.LossState(rec_dist=rec_dist, steps_anneal=HP["reg_anneal"]); st64.n_train_steps = step
        with O.gates(gates):
            _, _, grads64, _ = R.semi_iteration_grads(hp, st64, O.clone_params(p_step, dtype=torch.float64, requires_grad=True),
                                                      data.double(), eps.double(), rows)
        for k, p in model.named_parameters():
            check(p.grad, grads64[k], rtol=G_RTOL, atol_rel=G_ATOL, what="%s step %d grad vs gate-matched fp64 %s" % (kind, step, k))
        if step == 0:
            assert list(storer.keys()) == list(ref_logs.keys()), (list(storer.keys()), list(ref_logs.keys()))
            for k in ref_logs:
                np.testing.assert_allclose(storer[k][0], ref_logs[k].item(), rtol=5e-5, atol=1e-6, err_msg=k)
            assert storer["sup_loss"][0] > 0 and storer["n_labelled"][0] == B - B // 2
        else:
            assert len(storer) == 0
    assert loss_f.n_train_steps == 3


def _steps(hp, img, D, B, replay=None, poisoned=False, n=3, labels="rows", loss="s2vae"):
    """n seeded training steps -> (losses, parameters, gradients, loss object).  labels: "rows" (they and the position of the
    labelled rows change every step), "none" (labels=None), "negative" (a tensor without a labelled row), "off" (not passed)."""
    model, opt, loss_f = _native(hp, img, D, 33, 5e-4, loss)
    loss_f.replay = replay
    gen = torch.Generator().manual_seed(8)
    data = torch.empty((B,) + img, device=DEV)                                    # a plan is keyed on the batch's address
    losses = []
    patterns = ("second_half", "alternating", "last", "all")
    for i in range(n):
        data.copy_(torch.rand((B,) + img, generator=gen))
        eps = torch.randn(B, D, generator=gen).to(DEV)
        if poisoned:
            paths = _poison(model, loss_f)
            assert any("semi_dmu" in p for p in paths) or len(losses) == 0
        kw = {}
        if labels == "rows":
            kw = dict(labels=torch.tensor(_rows(B, i, patterns[i % 4]), device=DEV))
        elif labels == "none":
            kw = dict(labels=None)
        elif labels == "negative":
            kw = dict(labels=torch.tensor(_rows(B, i, "none"), device=DEV))
        losses.append(loss_f.fused_step(data, model, opt, None, eps=eps, **kw).item())
    torch.cuda.synchronize()
    grads = torch.cat([model.arena.view(k, grad=True).reshape(-1) for k in model.arena.shapes])
    return losses, model.arena.flat.clone(), grads.clone(), loss_f


def _same(a, b, what):
    assert a[0] == b[0], "%s: losses %s vs %s" % (what, a[0], b[0])
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), what + ": parameters or gradients differ"


def _hp(kind, **kw):
    return dict({k: v for k, v in HP.items()}, sup_loss=kind, gamma_sup=GAMMA[kind], **kw)


@pytest.mark.parametrize("kind", R.KINDS)
def test_an_all_unlabelled_batch_is_the_betaH_step_bit_for_bit(kind):
    img, D, B = (1, 32, 32), 10, 16
    plain = _steps(HP, img, D, B, labels="off", loss="betaH")
    _same(plain, _steps(_hp(kind), img, D, B, labels="none"), "labels=None")
    _same(plain, _steps(_hp(kind), img, D, B, labels="negative"), "a rows tensor without a labelled row")
    assert _steps(_hp(kind), img, D, B, labels="rows")[0] != plain[0]             # ... and labels do change the step


@pytest.mark.parametrize("kind,img,D,B", [("xent", (1, 32, 32), 10, 16), ("cov", (3, 64, 64), 10, 12), ("l2", (1, 32, 32), 20, 16)])
def test_eager_plan_graph_and_auto_give_the_same_bits(kind, img, D, B):
    """The rows, the position of the labelled rows and the annealed weight change every step: a row table or a weight frozen into
    a plan or a hipGraph shows here."""
    n = 6                                                                         # graph: the allocating step, two warm-up steps, the capture, two replays
    hp = _hp(kind, sup_anneal="anneal", sup_anneal_steps=8)
    eager = _steps(hp, img, D, B, None, n=n)
    assert all(np.isfinite(eager[0]))
    fixed = _steps(_hp(kind), img, D, B, None, n=n)
    assert eager[0] != fixed[0]                                                   # the annealed weight matters
    for mode in ("plan", "graph", "auto"):
        got = _steps(hp, img, D, B, mode, n=n)
        _same(eager, got, "%s vs eager" % mode)
        if mode != "auto":
            assert got[3]._graphs.replays >= 2, "%s: the step was never replayed" % mode


@pytest.mark.parametrize("kind", R.KINDS)
def test_poisoned_buffers_change_no_bit(kind):
    img, D, B = (1, 32, 32), 10, 16
    clean = _steps(_hp(kind), img, D, B)
    _same(clean, _steps(_hp(kind), img, D, B, poisoned=True), "poisoned engine buffers")
    _same(clean, _steps(_hp(kind), img, D, B, "plan", poisoned=True, n=3), "poisoned buffers under plan replay")


@pytest.mark.parametrize("kind", R.KINDS)
def test_eval_mode_computes_the_value_only(kind):
    img, B, D = (1, 32, 32), 6, 10
    model, opt, loss_f = _native(_hp(kind), img, D, 5, 5e-4)
    model.eval()
    gen = torch.Generator().manual_seed(2)
    data = torch.rand((B,) + img, generator=gen)
    rows = _rows(B, 0, "alternating")
    p = {k: v.detach().cpu().double() for k, v in model.named_parameters()}
    mu, logvar = O.encoder_forward(p, data.double())
    recon = O.decoder_forward(p, mu)
    kl, _ = O.kl_normal_loss(mu, logvar)
    Rv = R.regulariser_torch(mu, rows, R.DSPRITES, kind)
    want = O.reconstruction_loss(data.double(), recon) + 4 * kl + GAMMA[kind] * Rv          # evaluation: no annealing
    calls = []
    real = _semilib.call
    _semilib.call = lambda name, *a: (calls.append((name, a)), real(name, *a))[1]
    try:
        storer = defaultdict(list)
        out = loss_f.fused_step(dev(data), model, None, storer, labels=torch.tensor(rows, device=DEV))
    finally:
        _semilib.call = real
    np.testing.assert_allclose(out.item(), want.item(), rtol=2e-5)
    np.testing.assert_allclose(storer["sup_loss"][0], Rv.item(), rtol=1e-5)
    assert storer["n_labelled"][0] == 3
    grad_args = [a for name, a in calls if name == "dvae_semi_grad"]
    assert [name for name, _ in calls] == ["dvae_semi_partials", "dvae_semi_grad"] and grad_args[0][12] is None
    assert loss_f.n_train_steps == 0

    class _Loader(list):
        pass
    ev = Evaluator(model, loss_f, device=torch.device(DEV), is_progress_bar=False)
    losses = ev.compute_losses(_Loader([(data, torch.tensor(rows))]))
    assert list(losses) == list(storer) and losses["sup_loss"] == storer["sup_loss"][0] and losses["loss"] == out.item()
    unlabelled = ev.compute_losses(_Loader([(data, 0)]))
    assert unlabelled["sup_loss"] == 0.0 and unlabelled["n_labelled"] == 0.0


@pytest.mark.parametrize("kind", R.KINDS)
def test_autograd_signature_gives_the_fused_steps_gradients(kind):
    """loss(data, recon, latent_dist, is_train, storer, labels=) through torch.autograd against fused_step on a twin: the bound of
    test_gpu_step.py::test_autograd_path_after_fused_step_does_not_double_gradients."""
    img, B, D = (1, 64, 64), 6, 10
    m, o, l = _native(_hp(kind), img, D, 7, 5e-4)
    m2, o2, l2 = _native(_hp(kind), img, D, 7, 5e-4)
    gen = torch.Generator().manual_seed(3)
    data, eps = dev(torch.rand((B,) + img, generator=gen)), dev(torch.randn(B, D, generator=gen))
    rows = torch.tensor(_rows(B, 0, "alternating"), device=DEV)
    recon, latent_dist, z = m(data, eps=eps)
    storer = defaultdict(list)
    out = l(data, recon, latent_dist, True, storer, latent_sample=z, labels=rows)
    o.zero_grad(set_to_none=False)
    out.backward()
    storer2 = defaultdict(list)
    out2 = l2.fused_step(data, m2, o2, storer2, eps=eps, labels=rows)
    np.testing.assert_allclose(out.item(), out2.item(), rtol=2e-5)
    assert list(storer) == list(storer2)
    np.testing.assert_allclose(storer["sup_loss"][0], storer2["sup_loss"][0], rtol=1e-6)
    assert storer["n_labelled"][0] == storer2["n_labelled"][0] == 3
    for (k, p), (_, p2) in zip(m.named_parameters(), m2.named_parameters()):
        check(p.grad, p2.grad, rtol=1e-5, atol_rel=4e-6, what="autograd path vs fused step " + k)


def test_two_epochs_of_trainer_and_sup_loss_falls(tmp_path):
    sizes = (3, 4, 4)
    n = 48
    vals = R.values(np.arange(n), sizes, range(3))
    images = np.zeros((n, 1, 32, 32), np.uint8)
    for i, (a, b, c) in enumerate(vals):                                          # a bar whose grey level, row and column are the factors
        images[i, 0, 4 + 6 * b:10 + 6 * b, 4 + 6 * c:10 + 6 * c] = 85 * (a + 1)
    torch.manual_seed(0)
    model = init_specific_model("Burgess", (1, 32, 32), 10)
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    hp = dict(HP, n_data=n, lat_sizes=sizes, sup_loss="l2", gamma_sup=200.0, sup_reduction="mean")
    loss_f = get_loss_f("s2vae", device=torch.device(DEV), latent_dim=10, **hp)
    loss_f.record_loss_every = 2                                                  # every odd step logs
    loader = LabelledFactorLoader(torch.tensor(images), sizes, batch_size=4, n_labelled=16, seed=1, device=DEV)
    trainer = Trainer(model, opt, loss_f, device=torch.device(DEV), save_dir=str(tmp_path), is_progress_bar=False)
    trainer(loader, epochs=2)
    log = [line.strip().split(",") for line in open(tmp_path / "train_losses.log")][1:]
    sup = {int(e): float(v) for e, k, v in log if k == "sup_loss"}
    lab = {int(e): float(v) for e, k, v in log if k == "n_labelled"}
    print("sup_loss per epoch:", sup)
    assert lab == {0: 4.0, 1: 4.0} and loss_f.n_train_steps == 24
    assert np.isfinite(sup[0]) and sup[1] < sup[0]
