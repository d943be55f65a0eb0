"""-m gpu: the DIP-VAE I / II losses -- libdvae_dip_hip.so through its C-ABI against the fp64 restatement (tests/dip_ref.py), and
whole training steps of DipVaeLoss against the oracle.

Kernel level.  B in {1, 2, 3, 33} and one row on either side of every dispatch macro (DVAE_DIP_BLOCK_ROWS: one workgroup / two;
DVAE_DIP_BLOCK_ROWS * DVAE_DIP_MAX_GROUPS: the first size at which a workgroup makes a second trip), D in {1, 2, 10, 16, 17, 40,
128}, both types, the three tables of dip_ref (Gaussian; the offset family 30 + 1e-3 noise, which a raw-moment fp32 sum fails; the
trained regime).  C is bitwise symmetric and inside 8 B 2^-53 sqrt(m2_d m2_e); values and gradients are inside the first-order
bounds of dip_ref.tolerances, whose fp32 part carries the margin max(1, 4 e32) = 20 (e32 = 5.0: dip_ref.E32_WORST, measured on
the CPU and pinned by tests/test_dip_host.py).  Every case prints the worst error / bound at margin 1 before it asserts.

Whole step, shaped like test_gpu_step.py::test_fused_step_vs_oracle, same tolerances: loss 2e-5; gradients rtol 1e-5 + 2e-6
max|g| against the gate-matched fp64 oracle at the engine's parameters, three steps, no outliers.
"""
import functools
from collections import defaultdict

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import dip_ref as R
from gpu_util import DEV, check, dev, stream
from guard_util import Guarded, run_contract
from oracle import disvae_oracle as O
from oracle.gate_match import engine_gates, gate_mismatches
from disvae_amd import _diplib, _lib
from disvae_amd import schedule as SCHED
from disvae_amd.evaluate import Evaluator
from disvae_amd.models.losses import get_loss_f
from disvae_amd.models.vae import init_specific_model
from test_gpu_step_poison import _poison

EDGE = _diplib.BLOCK_ROWS * _diplib.MAX_GROUPS
SHAPES_B = (1, 2, 3, 33, _diplib.BLOCK_ROWS, EDGE, EDGE + 1)
SHAPES_D = (1, 2, 10, 16, 17, 40, 128)
LAMBDA_OD = 10.0


@functools.lru_cache(maxsize=None)
def _reference(kind, B, D, dip_type):
    """(mu, logvar, restatement, bounds): computed once, shared by the tests, never written to."""
    lam_d = R.default_lambda_d_factor(dip_type) * LAMBDA_OD
    mu, lv = R.table(kind, B, D)
    ref = R.regulariser(mu, lv, dip_type, LAMBDA_OD, lam_d)
    return mu, lv, ref, R.tolerances(ref, LAMBDA_OD, lam_d, margin=R.MARGIN), R.tolerances(ref, LAMBDA_OD, lam_d, margin=1.0), lam_d


def _launch(mu, lv, dip_type, lam_d, grads=True, loss0=None):
    """The two launches on device copies -> (out fp64 [3 + D D], dmu, dlv, loss_io) as numpy."""
    B, D = mu.shape
    dmu_t = torch.tensor(mu, device=DEV)
    lv_t = torch.tensor(lv, device=DEV) if dip_type == "ii" else None
    ws = torch.full((_diplib.ws_doubles(B, D),), float("nan"), dtype=torch.float64, device=DEV)
    out = torch.full((_diplib.out_doubles(D),), float("nan"), dtype=torch.float64, device=DEV)
    gmu = torch.full((B, D), float("nan"), device=DEV) if grads else None
    glv = torch.full((B, D), float("nan"), device=DEV) if grads and lv_t is not None else None
    lio = None if loss0 is None else torch.tensor([loss0], dtype=torch.float32, device=DEV)
    p = lambda t: None if t is None else t.data_ptr()
    _diplib.call("dvae_dip_moments", p(dmu_t), p(lv_t), B, D, p(ws), stream())
    _diplib.call("dvae_dip_grad", p(dmu_t), p(lv_t), B, D, LAMBDA_OD, lam_d, p(ws), p(gmu), p(glv), p(out), p(lio), stream())
    torch.cuda.synchronize()
    n = lambda t: None if t is None else t.cpu().numpy()
    return n(out), n(gmu), n(glv), n(lio)


@pytest.mark.parametrize("dip_type", R.TYPES)
@pytest.mark.parametrize("kind", R.TABLES)
def test_kernels_against_the_restatement(kind, dip_type):
    worst = dict(C=0.0, R=0.0, dmu=0.0, dlv=0.0)
    for B in SHAPES_B:
        for D in SHAPES_D:
            mu, lv, ref, tol, tol1, lam_d = _reference(kind, B, D, dip_type)
            out, gmu, glv, lio = _launch(mu, lv, dip_type, lam_d, loss0=3.25)
            C = out[3:].reshape(D, D)
            what = "%s %s B=%d D=%d" % (kind, dip_type, B, D)
            assert np.isfinite(out).all() and np.isfinite(gmu).all(), what
            assert C.tobytes() == C.T.copy().tobytes(), what + ": C is not bitwise symmetric"
            ratios = dict(C=np.abs(C - ref["C"]) / (tol["C"] + 1e-300),
                          R=np.abs(out[:3] - [ref["R"], ref["R_od"], ref["R_d"]]) / (tol["R"] + 1e-300),
                          dmu=np.abs(gmu - ref["dmu"]) / (tol1["dmu"] + 1e-300))
            if dip_type == "ii":
                ratios["dlv"] = np.abs(glv - ref["dlv"]) / (tol1["dlv"] + 1e-300)
            else:
                assert glv is None
            for k, v in ratios.items():
                worst[k] = max(worst[k], float(v.max()))
            assert (np.abs(C - ref["C"]) <= tol["C"]).all(), what + ": C"           # (B = 1: the bound of type I is zero, and so is C)
            assert (np.abs(out[:3] - [ref["R"], ref["R_od"], ref["R_d"]]) <= tol["R"]).all(), what + ": R"
            assert (np.abs(gmu - ref["dmu"]) <= tol["dmu"]).all(), what + ": dmu %.3g x the bound at margin 1" % ratios["dmu"].max()
            if dip_type == "ii":
                assert (np.abs(glv - ref["dlv"]) <= tol["dlv"]).all(), what + ": dlv %.3g x the bound at margin 1" % ratios["dlv"].max()
            if D == 1:
                assert out[1] == 0.0                                                     # no off-diagonal pair
            # loss_io is changed by exactly + R (one fp32 add of the rounded value)
            assert lio[0] == np.float32(3.25) + np.float32(out[0]), what
            assert abs(out[0] - (out[1] + out[2])) <= 2 * R.U * abs(out[0])              # (the compiler may fuse the last multiply into the add)
    print("%s %s: worst error / bound -- C %.3g, R %.3g, dmu %.3g and dlv %.3g at margin 1 (allowed: %g)"
          % (kind, dip_type, worst["C"], worst["R"], worst["dmu"], worst["dlv"], R.MARGIN))


@pytest.mark.parametrize("dip_type", R.TYPES)
def test_two_runs_and_the_value_only_launch_give_the_same_bits(dip_type):
    for B, D in ((3, 2), (33, 10), (EDGE + 1, 17), (EDGE + 1, 128)):
        mu, lv, ref, tol, _, lam_d = _reference("regime", B, D, dip_type)
        a = _launch(mu, lv, dip_type, lam_d, loss0=-1.5)
        b = _launch(mu, lv, dip_type, lam_d, loss0=-1.5)
        for x, y in zip(a, b):
            assert (x is None and y is None) or x.tobytes() == y.tobytes(), (B, D)
        value_only = _launch(mu, lv, dip_type, lam_d, grads=False)
        assert value_only[0].tobytes() == a[0].tobytes() and value_only[1] is None and value_only[3] is None


def test_a_latent_dimension_above_the_limit_is_refused():
    t = torch.zeros(4 * 129, device=DEV)
    w = torch.zeros(1 << 16, dtype=torch.float64, device=DEV)
    for name, args in (("dvae_dip_moments", (t.data_ptr(), None, 4, 129, w.data_ptr(), stream())),
                       ("dvae_dip_grad", (t.data_ptr(), None, 4, 129, 1.0, 1.0, w.data_ptr(), None, None, w.data_ptr(), None, stream()))):
        with pytest.raises(_lib.DvaeHipError, match="invalid argument.*DVAE_DIP_MAX_D"):
            _diplib.call(name, *args)
    assert _diplib.lib().dvae_dip_ws_doubles(4, 129) == 0
    torch.cuda.synchronize()
    assert not t.any() and not w.any()


def _dip_call(name):
    return lambda args: _diplib.call(name, *[a.ptr if isinstance(a, Guarded) else a for a in args])


@pytest.mark.parametrize("dip_type", R.TYPES)
@pytest.mark.parametrize("B,D", [(3, 2), (33, 10), (EDGE + 1, 17), (40, 128)])
def test_memory_contract(B, D, dip_type):
    """Guard-banded, NaN-poisoned buffers at 256-byte alignment and at the weakest the header promises (4 bytes for the fp32
    arguments, 8 for ws and out): guards untouched, inputs unchanged, every defined output written, the same bits in all runs."""
    mu, lv, ref, tol, _, lam_d = _reference("gauss", B, D, dip_type)
    two = dip_type == "ii"
    groups = _diplib.groups(B)[0]
    rec = np.zeros((groups, 2 * D + D * D), dtype=bool)
    rec[:, :D] = True
    rec[:, D:2 * D] = two
    rec[:, 2 * D:] = np.triu(np.ones((D, D), dtype=bool)).reshape(-1)
    defined = torch.tensor(rec.reshape(-1))

    def moments(al):
        return [al.inp("mu", mu, align=4), al.inp("logvar", lv, align=4) if two else None, B, D,
                al.out("ws", (groups * (2 * D + D * D),), dtype=torch.float64, align=8, written=defined), stream()]
    runs = run_contract("dvae_dip_moments", moments, fn=_dip_call("dvae_dip_moments"))
    ws = runs[0].args[-1].t.clone()
    ws[~defined.to(ws.device)] = float("nan")                             # what the first launch leaves undefined is never read

    def grad(al):
        return [al.inp("mu", mu, align=4), al.inp("logvar", lv, align=4) if two else None, B, D, LAMBDA_OD, lam_d,
                al.inp("ws", ws, align=8, dtype=torch.float64), al.out("dmu", (B, D), align=4),
                al.out("dlv", (B, D), align=4) if two else None, al.out("out", (3 + D * D,), dtype=torch.float64, align=8),
                al.inout("loss_io", torch.tensor([2.5]), align=4), stream()]
    runs = run_contract("dvae_dip_grad", grad, fn=_dip_call("dvae_dip_grad"))
    got = {g.name: g.t.cpu().numpy() for g in runs[2].args}
    assert (np.abs(got["dmu"] - ref["dmu"]) <= tol["dmu"]).all()
    assert got["loss_io"][0] == np.float32(2.5) + np.float32(got["out"][0])


# ---- whole steps ------------------------------------------------------------------------------------------------------------------
HP = dict(rec_dist="bernoulli", reg_anneal=10000, betaH_B=4, betaB_initC=0, betaB_finC=25, betaB_G=1000, factor_G=6.4,
          lr_disc=1e-4, btcvae_A=1, btcvae_B=6.4, btcvae_G=1, n_data=202599)
G_RTOL, G_ATOL = 1e-5, 2e-6
STEP_CASES = [("dipI", (1, 32, 32), 8, 10, "bernoulli"), ("dipII", (3, 64, 64), 5, 10, "gaussian"), ("dipII", (1, 64, 64), 33, 10, "bernoulli"),
              ("dipI", (1, 32, 32), 9, 20, "bernoulli"), ("dipII", (3, 64, 64), 2, 10, "bernoulli")]


def _native(loss, img, D, seed, lr, rec_dist="bernoulli"):
    torch.manual_seed(seed)
    model = init_specific_model("Burgess", img, D)
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    loss_f = get_loss_f(loss, device=torch.device(DEV), latent_dim=D, **dict(HP, rec_dist=rec_dist))
    model.to(DEV)
    model.train()
    return model, opt, loss_f


@pytest.mark.parametrize("loss,img,B,D,rec_dist", STEP_CASES)
def test_fused_step_vs_oracle(loss, img, B, D, rec_dist):
    seed, lr = 1234, 5e-4
    model, opt, loss_f = _native(loss, img, D, seed, lr, rec_dist)
    hp = dict(HP, latent_dim=D)
    gen = torch.Generator().manual_seed(seed + 1)
    for step in range(3):
        data = torch.rand((B,) + tuple(img), generator=gen)
        eps = torch.randn(B, D, generator=gen)
        p_step = {k: p.detach().cpu().clone() for k, p in model.named_parameters()}
        st = O.LossState(rec_dist=rec_dist, steps_anneal=HP["reg_anneal"]); st.n_train_steps = step
        ref_loss, ref_logs, _, ref_outs = R.dip_iteration_grads(loss, hp, st, O.clone_params(p_step, requires_grad=True), data, eps)
        storer = defaultdict(list)
        out = loss_f.fused_step(dev(data), model, opt, storer, eps=dev(eps))
        buf = model.engine.buffers(B)
        print("%s step %d: loss %.6f (oracle %.6f), dip %.6f" % (loss, step, out.item(), ref_loss.item(), ref_logs["dip_loss"].item()))
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
            _, _, grads64, _ = R.dip_iteration_grads(loss, hp, st64, O.clone_params(p_step, dtype=torch.float64, requires_grad=True),
                                                     data.double(), eps.double())
        for k, p in model.named_parameters():
            check(p.grad, grads64[k], rtol=G_RTOL, atol_rel=G_ATOL, what="%s step %d grad vs gate-matched fp64 %s" % (loss, step, k))
        if step == 0:
            assert list(storer.keys()) == list(ref_logs.keys()), (list(storer.keys()), list(ref_logs.keys()))
            for k in ref_logs:
                np.testing.assert_allclose(storer[k][0], ref_logs[k].item(), rtol=5e-5, atol=1e-6, err_msg=k)
            assert storer["dip_loss"][0] > 0
        else:
            assert len(storer) == 0
    assert loss_f.n_train_steps == 3


@pytest.mark.parametrize("loss", ["dipI", "dipII"])
def test_eval_mode_computes_the_value_only(loss):
    img, B, D = (1, 32, 32), 6, 10
    model, opt, loss_f = _native(loss, img, D, 5, 5e-4)
    model.eval()
    gen = torch.Generator().manual_seed(2)
    data = torch.rand((B,) + img, generator=gen)
    p = {k: v.detach().cpu().double() for k, v in model.named_parameters()}
    mu, logvar = O.encoder_forward(p, data.double())
    recon = O.decoder_forward(p, mu)
    kl, _ = O.kl_normal_loss(mu, logvar)
    Rv = R.regulariser_torch(mu, logvar, loss_f.dip_type, loss_f.lambda_od, loss_f.lambda_d)
    want = O.reconstruction_loss(data.double(), recon) + kl + Rv                  # evaluation: no annealing
    calls = []
    real = _diplib.call
    _diplib.call = lambda name, *a: (calls.append((name, a)), real(name, *a))[1]
    try:
        storer = defaultdict(list)
        out = loss_f.fused_step(dev(data), model, None, storer)
    finally:
        _diplib.call = real
    np.testing.assert_allclose(out.item(), want.item(), rtol=2e-5)
    np.testing.assert_allclose(storer["dip_loss"][0], Rv.item(), rtol=1e-5)
    grad_args = [a for name, a in calls if name == "dvae_dip_grad"]
    assert [name for name, _ in calls] == ["dvae_dip_moments", "dvae_dip_grad"] and grad_args[0][7] is None and grad_args[0][8] is None
    assert loss_f.n_train_steps == 0

    class _Loader(list):
        pass
    ev = Evaluator(model, loss_f, device=torch.device(DEV), is_progress_bar=False)
    losses = ev.compute_losses(_Loader([(data, None)]))
    assert list(losses) == list(storer) and losses["dip_loss"] == storer["dip_loss"][0] and losses["loss"] == out.item()


def _steps(loss, img, D, B, replay=None, poisoned=False, single=False, n=3, lam_od=None):
    """n seeded training steps -> (losses, parameters, gradients)."""
    model, opt, loss_f = _native(loss, img, D, 33, 5e-4)
    loss_f.replay = replay
    if lam_od is not None:
        loss_f.lambda_od = lam_od
    if single:
        sw = tuple("1" if name == "DVAE_STREAMS" else v for (name, _), v in zip(SCHED.SWITCHES, SCHED.switches()))
        pol = SCHED.build_policy(tuple(img), D, B, sw, 1, loss_f.KIND, True, None)
        assert pol.single_stream
        loss_f.policy_override = pol._asdict()
    gen = torch.Generator().manual_seed(8)
    data = torch.empty((B,) + img, device=DEV)                                    # a plan is keyed on the batch's address
    losses = []
    for _ in range(n):
        data.copy_(torch.rand((B,) + img, generator=gen))
        eps = torch.randn(B, D, generator=gen).to(DEV)
        if poisoned:
            paths = _poison(model, loss_f)
            assert any("dip_dmu" in p for p in paths) or len(losses) == 0
        losses.append(loss_f.fused_step(data, model, opt, None, eps=eps).item())
    torch.cuda.synchronize()
    grads = torch.cat([model.arena.view(k, grad=True).reshape(-1) for k in model.arena.shapes])
    return losses, model.arena.flat.clone(), grads.clone(), loss_f


def _same(a, b, what):
    assert a[0] == b[0], "%s: losses %s vs %s" % (what, a[0], b[0])
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), what + ": parameters or gradients differ"


@pytest.mark.parametrize("loss,img,D,B", [("dipI", (1, 32, 32), 10, 8), ("dipII", (3, 64, 64), 10, 5), ("dipII", (1, 32, 32), 20, 9)])
def test_eager_plan_graph_and_auto_give_the_same_bits(loss, img, D, B):
    n = 6                                                                         # graph: the allocating step, two warm-up steps, the capture, two replays
    eager = _steps(loss, img, D, B, None, n=n)
    assert all(np.isfinite(eager[0]))
    for mode in ("plan", "graph", "auto"):
        got = _steps(loss, img, D, B, mode, n=n)
        _same(eager, got, "%s vs eager" % mode)
        if mode != "auto":
            assert got[3]._graphs.replays >= 2, "%s: the step was never replayed" % mode


def test_the_hyper_parameters_join_the_replay_key():
    loss, img, D, B = "dipII", (1, 32, 32), 10, 8
    model, opt, loss_f = _native(loss, img, D, 33, 5e-4)
    loss_f.replay = "plan"
    gen = torch.Generator().manual_seed(8)
    data = torch.rand((B,) + img, generator=gen).to(DEV)
    eps = torch.randn(B, D, generator=gen).to(DEV)
    for _ in range(3):
        loss_f.fused_step(data, model, opt, None, eps=eps)
    replays = loss_f._graphs.replays
    assert replays >= 1
    loss_f.lambda_od = 3.0                                                        # a recorded launch froze the old value
    storer = defaultdict(list)
    loss_f.n_train_steps = 50                                                     # the next step logs
    loss_f.fused_step(data, model, opt, storer, eps=eps)
    assert loss_f._graphs.replays == replays
    buf = model.engine.buffers(B)
    want = R.regulariser(buf.mu.cpu().numpy(), buf.logvar.cpu().numpy(), "ii", 3.0, 3.0)["R"]
    np.testing.assert_allclose(storer["dip_loss"][0], want, rtol=1e-5)


@pytest.mark.parametrize("loss,img,D,B", [("dipI", (1, 32, 32), 10, 8), ("dipII", (1, 32, 32), 20, 9)])
def test_poisoned_buffers_and_the_single_stream_policy_change_no_bit(loss, img, D, B):
    clean = _steps(loss, img, D, B)
    _same(clean, _steps(loss, img, D, B, poisoned=True), "poisoned engine buffers")
    _same(clean, _steps(loss, img, D, B, single=True), "single-stream policy")
    _same(clean, _steps(loss, img, D, B, "plan", poisoned=True, n=3), "poisoned buffers under plan replay")


@pytest.mark.parametrize("loss", ["dipI", "dipII"])
def test_autograd_signature_gives_the_fused_steps_gradients(loss):
    """loss(data, recon, latent_dist, is_train, storer) through torch.autograd against fused_step on a twin: the bound of
    test_gpu_step.py::test_autograd_path_after_fused_step_does_not_double_gradients."""
    img, B, D = (1, 64, 64), 6, 10
    m, o, l = _native(loss, img, D, 7, 5e-4)
    m2, o2, l2 = _native(loss, img, D, 7, 5e-4)
    gen = torch.Generator().manual_seed(3)
    data, eps = dev(torch.rand((B,) + img, generator=gen)), dev(torch.randn(B, D, generator=gen))
    recon, latent_dist, z = m(data, eps=eps)
    storer = defaultdict(list)
    out = l(data, recon, latent_dist, True, storer, latent_sample=z)
    o.zero_grad(set_to_none=False)
    out.backward()
    storer2 = defaultdict(list)
    out2 = l2.fused_step(data, m2, o2, storer2, eps=eps)
    np.testing.assert_allclose(out.item(), out2.item(), rtol=2e-5)
    assert list(storer) == list(storer2)
    np.testing.assert_allclose(storer["dip_loss"][0], storer2["dip_loss"][0], rtol=1e-6)
    for (k, p), (_, p2) in zip(m.named_parameters(), m2.named_parameters()):
        check(p.grad, p2.grad, rtol=1e-5, atol_rel=4e-6, what="autograd path vs fused step " + k)
