"""-m gpu: the InfoVAE / MMD-VAE loss -- libdvae_mmd_hip.so through its C-ABI against the fp64 restatement (tests/mmd_ref.py), and
whole training steps of InfoVaeLoss against the oracle.

Kernel level.  B in {1, 2, 3, 33} and one row on either side of every tiling macro (DVAE_MMD_ROWS: one row tile / two, and 2 B
crosses DVAE_MMD_COLS there; DVAE_MMD_COLS: a p tile's second column chunk; DVAE_MMD_COLS * DVAE_MMD_MAX_CGROUPS / 2 and
DVAE_MMD_COLS * DVAE_MMD_MAX_CGROUPS: the first sizes at which a z tile and a p tile make a second trip), D in {1, 2, 10, 16, 17,
40, 128} (the kernels have no switch in D), both kernels, the four tables of mmd_ref (Gaussian; the trained regime, where RBF
terms underflow; the offset family 30 + 1e-3 noise, which |a|^2 + |b|^2 - 2 a.b fails; ties).  The three fp64 sums are inside the
accumulation bounds of mmd_ref.tolerances (first order in the fp32 evaluation of k, from sum |terms|); the gradients are inside
its first-order bounds, whose fp32 part carries the margin max(1, 4 e32) = 3.72 (e32 = 0.93: mmd_ref.E32_WORST, measured on the
CPU and pinned by tests/test_mmd_host.py).  Every case prints the worst error / bound at margin 1 before it asserts.

Whole step, shaped like test_gpu_step.py::test_fused_step_vs_oracle, same tolerances: loss 2e-5; gradients rtol 1e-5 + 2e-6
max|g| against the gate-matched fp64 oracle at the engine's parameters, three steps, eps and the prior draws injected.
"""
import functools
from collections import defaultdict

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mmd_ref as R
from gpu_util import DEV, check, dev, stream
from guard_util import Guarded, run_contract
from oracle import disvae_oracle as O
from oracle.gate_match import engine_gates, gate_mismatches
from disvae_amd import _lib, _mmdlib
from disvae_amd.evaluate import Evaluator
from disvae_amd.models.losses import get_loss_f
from disvae_amd.models.vae import init_specific_model
from test_gpu_step_poison import _poison

TRIP_Z = _mmdlib.COLS * _mmdlib.MAX_CGROUPS // 2
TRIP_P = _mmdlib.COLS * _mmdlib.MAX_CGROUPS
SHAPES_B = (1, 2, 3, 33, _mmdlib.ROWS, _mmdlib.ROWS + 1, _mmdlib.COLS, TRIP_Z, TRIP_Z + 1, TRIP_P, TRIP_P + 1)
SHAPES_D = (1, 2, 10, 16, 17, 40, 128)
W = 999.0                                                     # alpha + lam - 1 at the defaults


@functools.lru_cache(maxsize=None)
def _reference(tab, B, D, kind):
    """(z, p, mu, restatement, bounds at the margin, bounds at margin 1, h): computed once, shared by the tests, never written to."""
    z, p, mu = R.table(tab, B, D)
    h = R.default_bandwidth(D)
    ref = R.mmd(z, p, kind, h, W, mu)
    return z, p, mu, ref, R.tolerances(ref, margin=R.MARGIN), R.tolerances(ref, margin=1.0), h


def _launch(z, p, mu, kind, h, grads=True, loss0=None, w=W):
    """The two launches on device copies -> (out fp64 [5], dmu, dlv, loss_io) as numpy."""
    B, D = z.shape
    z_t, p_t, mu_t = (torch.tensor(a, device=DEV) for a in (z, p, mu))
    ws = torch.full((_mmdlib.ws_doubles(B, D),), float("nan"), dtype=torch.float64, device=DEV)
    out = torch.full((_mmdlib.OUT_DOUBLES,), float("nan"), dtype=torch.float64, device=DEV)
    gmu = torch.full((B, D), float("nan"), device=DEV) if grads else None
    glv = torch.full((B, D), float("nan"), device=DEV) if grads else None
    lio = None if loss0 is None else torch.tensor([loss0], dtype=torch.float32, device=DEV)
    q = lambda t: None if t is None else t.data_ptr()
    _mmdlib.call("dvae_mmd_pairs", q(z_t), q(p_t), B, D, _mmdlib.KERNELS[kind], h, int(grads), q(ws), stream())
    _mmdlib.call("dvae_mmd_finish", q(z_t), q(mu_t), B, D, w, q(ws), q(gmu), q(glv), q(out), q(lio), stream())
    torch.cuda.synchronize()
    n = lambda t: None if t is None else t.cpu().numpy()
    return n(out), n(gmu), n(glv), n(lio)


@pytest.mark.parametrize("kind", R.KERNELS)
@pytest.mark.parametrize("tab", R.TABLES)
def test_kernels_against_the_restatement(tab, kind):
    worst = dict(S=0.0, mmd=0.0, dmu=0.0, dlv=0.0)
    for B in SHAPES_B:
        for D in SHAPES_D:
            z, p, mu, ref, tol, tol1, h = _reference(tab, B, D, kind)
            out, gmu, glv, lio = _launch(z, p, mu, kind, h, loss0=3.25)
            what = "%s %s B=%d D=%d" % (tab, kind, B, D)
            assert np.isfinite(out).all() and np.isfinite(gmu).all() and np.isfinite(glv).all(), what
            want = np.array([ref["wmmd"], ref["mmd"], ref["S_zz"], ref["S_pp"], ref["S_zp"]])
            bound = np.array([tol["wmmd"], tol["mmd"], tol["S_zz"], tol["S_pp"], tol["S_zp"]])
            err = np.abs(out - want)
            ratios = dict(S=(err[2:] / (bound[2:] + 1e-300)).max(), mmd=(err[:2] / (bound[:2] + 1e-300)).max(),
                          dmu=(np.abs(gmu - ref["dmu"]) / (tol1["dmu"] + 1e-300)).max(),
                          dlv=(np.abs(glv - ref["dlv"]) / (tol1["dlv"] + 1e-300)).max())
            for k, v in ratios.items():
                worst[k] = max(worst[k], float(v))
            assert (err <= bound).all(), what + ": value sums, error / bound %s" % (err / (bound + 1e-300))
            assert (np.abs(gmu - ref["dmu"]) <= tol["dmu"]).all(), what + ": dmu %.3g x the bound at margin 1" % ratios["dmu"]
            assert (np.abs(glv - ref["dlv"]) <= tol["dlv"]).all(), what + ": dlv %.3g x the bound at margin 1" % ratios["dlv"]
            if B == 1:                                                                   # defined as 0, with zero gradients
                assert out[0] == 0.0 and out[1] == 0.0 and out[2] == 0.0 and out[3] == 0.0 and not gmu.any() and not glv.any()
            # loss_io is changed by exactly + w MMD_u (one fp32 add of the rounded value)
            assert lio[0] == np.float32(3.25) + np.float32(out[0]), what
            assert out[0] == W * out[1]
    print("%s %s: worst error / bound -- sums %.3g, MMD_u %.3g; dmu %.3g and dlv %.3g at margin 1 (allowed: %g)"
          % (tab, kind, worst["S"], worst["mmd"], worst["dmu"], worst["dlv"], R.MARGIN))


@pytest.mark.parametrize("kind", R.KERNELS)
def test_two_runs_and_the_value_only_launch_give_the_same_bits(kind):
    for B, D in ((1, 4), (3, 2), (33, 10), (TRIP_Z + 1, 17), (TRIP_P + 1, 128)):
        z, p, mu, ref, tol, _, h = _reference("regime", B, D, kind)
        a = _launch(z, p, mu, kind, h, loss0=-1.5)
        b = _launch(z, p, mu, kind, h, loss0=-1.5)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes(), (B, D)
        value_only = _launch(z, p, mu, kind, h, grads=False)
        assert value_only[0].tobytes() == a[0].tobytes() and value_only[1] is None and value_only[2] is None and value_only[3] is None


def test_a_latent_dimension_above_the_limit_is_refused():
    t = torch.zeros(4 * 129, device=DEV)
    w = torch.zeros(1 << 16, dtype=torch.float64, device=DEV)
    for name, args in (("dvae_mmd_pairs", (t.data_ptr(), t.data_ptr(), 4, 129, 1, 6.0, 1, w.data_ptr(), stream())),
                       ("dvae_mmd_finish", (t.data_ptr(), t.data_ptr(), 4, 129, 1.0, w.data_ptr(), None, None, w.data_ptr(), None, stream()))):
        with pytest.raises(_lib.DvaeHipError, match="invalid argument.*DVAE_MMD_MAX_D"):
            _mmdlib.call(name, *args)
    assert _mmdlib.lib().dvae_mmd_ws_doubles(4, 129) == 0
    torch.cuda.synchronize()
    assert not t.any() and not w.any()


def _mmd_call(name):
    return lambda args: _mmdlib.call(name, *[a.ptr if isinstance(a, Guarded) else a for a in args])


@pytest.mark.parametrize("kind", R.KERNELS)
@pytest.mark.parametrize("B,D", [(3, 2), (33, 10), (TRIP_Z + 1, 17), (40, 128)])
def test_memory_contract(B, D, kind):
    """Guard-banded, NaN-poisoned buffers at 256-byte alignment and at the weakest the header promises (4 bytes for the fp32
    arguments, 8 for ws and out): guards untouched, inputs unchanged, every defined output written, the same bits in all runs."""
    z, p, mu, ref, tol, _, h = _reference("gauss", B, D, kind)
    tiles, (gz, _cz), (gp, _cp) = _mmdlib.tiling(B)
    rec = np.zeros((2 * tiles, gz, 2), dtype=bool)
    rec[:tiles] = True
    rec[tiles:, :gp] = True                                                # a p tile has fewer column chunks
    defined = torch.tensor(np.concatenate([rec.reshape(-1), np.ones(B * gz * D, dtype=bool)]))
    assert defined.numel() == _mmdlib.ws_doubles(B, D)

    def pairs(al):
        return [al.inp("z", z, align=4), al.inp("p", p, align=4), B, D, _mmdlib.KERNELS[kind], h, 1,
                al.out("ws", (defined.numel(),), dtype=torch.float64, align=8, written=defined), stream()]
    runs = run_contract("dvae_mmd_pairs", pairs, fn=_mmd_call("dvae_mmd_pairs"))
    ws = runs[0].args[-1].t.clone()
    ws[~defined.to(ws.device)] = float("nan")                             # what the first launch leaves undefined is never read

    def finish(al):
        return [al.inp("z", z, align=4), al.inp("mu", mu, align=4), B, D, W, al.inp("ws", ws, align=8, dtype=torch.float64),
                al.out("dmu", (B, D), align=4), al.out("dlv", (B, D), align=4), al.out("out", (5,), dtype=torch.float64, align=8),
                al.inout("loss_io", torch.tensor([2.5]), align=4), stream()]
    runs = run_contract("dvae_mmd_finish", finish, fn=_mmd_call("dvae_mmd_finish"))
    got = {g.name: g.t.cpu().numpy() for g in runs[2].args}
    assert (np.abs(got["dmu"] - ref["dmu"]) <= tol["dmu"]).all() and (np.abs(got["dlv"] - ref["dlv"]) <= tol["dlv"]).all()
    assert abs(got["out"][1] - ref["mmd"]) <= tol["mmd"]
    assert got["loss_io"][0] == np.float32(2.5) + np.float32(got["out"][0])


# ---- whole steps ------------------------------------------------------------------------------------------------------------------
HP = dict(rec_dist="bernoulli", reg_anneal=10000, betaH_B=4, betaB_initC=0, betaB_finC=25, betaB_G=1000, factor_G=6.4,
          lr_disc=1e-4, btcvae_A=1, btcvae_B=6.4, btcvae_G=1, n_data=202599)
G_RTOL, G_ATOL = 1e-5, 2e-6
MMD_VAE = dict(info_alpha=1.0, info_lambda=100.0)                              # alpha = 1: no KL term at all
STEP_CASES = [((1, 32, 32), 8, 10, "bernoulli", dict(mmd_kernel="imq")), ((3, 64, 64), 5, 10, "gaussian", dict(mmd_kernel="rbf")),
              ((1, 64, 64), 33, 10, "bernoulli", dict(MMD_VAE, mmd_kernel="rbf", mmd_bandwidth=7.5)),
              ((1, 32, 32), 9, 20, "bernoulli", dict(info_alpha=0.5, info_lambda=10.0)), ((3, 64, 64), 2, 10, "bernoulli", dict())]


def _native(img, D, seed, lr, rec_dist="bernoulli", **info):
    torch.manual_seed(seed)
    model = init_specific_model("Burgess", img, D)
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    loss_f = get_loss_f("infovae", device=torch.device(DEV), latent_dim=D, **dict(HP, rec_dist=rec_dist, **info))
    model.to(DEV)
    model.train()
    return model, opt, loss_f


@pytest.mark.parametrize("img,B,D,rec_dist,info", STEP_CASES)
def test_fused_step_vs_oracle(img, B, D, rec_dist, info):
    seed, lr = 1234, 5e-4
    model, opt, loss_f = _native(img, D, seed, lr, rec_dist, **info)
    hp = dict(HP, latent_dim=D, **info)
    gen = torch.Generator().manual_seed(seed + 1)
    for step in range(3):
        data = torch.rand((B,) + tuple(img), generator=gen)
        eps = torch.randn(B, D, generator=gen)
        prior = torch.randn(B, D, generator=gen)
        p_step = {k: p.detach().cpu().clone() for k, p in model.named_parameters()}
        st = O.LossState(rec_dist=rec_dist, steps_anneal=HP["reg_anneal"]); st.n_train_steps = step
        ref_loss, ref_logs, _, ref_outs = R.mmd_iteration_grads(hp, st, O.clone_params(p_step, requires_grad=True), data, eps, prior)
        storer = defaultdict(list)
        out = loss_f.fused_step(dev(data), model, opt, storer, eps=dev(eps), prior=dev(prior))
        buf = model.engine.buffers(B)
        print("step %d: loss %.6f (oracle %.6f), mmd term %.6f" % (step, out.item(), ref_loss.item(), ref_logs["mmd_loss"].item()))
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
            _, _, grads64, _ = R.mmd_iteration_grads(hp, st64, O.clone_params(p_step, dtype=torch.float64, requires_grad=True),
                                                     data.double(), eps.double(), prior.double())
        for k, p in model.named_parameters():
            check(p.grad, grads64[k], rtol=G_RTOL, atol_rel=G_ATOL, what="step %d grad vs gate-matched fp64 %s" % (step, k))
        if step == 0:
            assert list(storer.keys()) == list(ref_logs.keys()), (list(storer.keys()), list(ref_logs.keys()))
            for k in ref_logs:                    # (mmd_loss is w times a difference of O(1) fp32 sums in the oracle: the loss's absolute slack)
                atol = 2e-5 * abs(ref_loss.item()) if k == "mmd_loss" else 1e-6
                np.testing.assert_allclose(storer[k][0], ref_logs[k].item(), rtol=5e-5, atol=atol, err_msg=k)
            assert storer["mmd_loss"][0] != 0
        else:
            assert len(storer) == 0
    assert loss_f.n_train_steps == 3


@pytest.mark.parametrize("kind", R.KERNELS)
def test_a_one_image_batch_is_zero_with_zero_gradients_through_autograd(kind):
    from disvae_amd.models.losses import _MmdFn
    z = torch.randn(1, 10, device=DEV, requires_grad=True)
    out = _MmdFn.apply(z, torch.randn(1, 10, device=DEV), kind, 20.0, 999.0)
    out.backward()
    assert out.item() == 0.0 and z.grad.shape == (1, 10) and not z.grad.any()


@pytest.mark.parametrize("kind", R.KERNELS)
def test_eval_mode_computes_the_value_only_and_draws_the_prior(kind):
    img, B, D = (1, 32, 32), 6, 10
    model, opt, loss_f = _native(img, D, 5, 5e-4, mmd_kernel=kind, info_alpha=0.25)
    model.eval()
    gen = torch.Generator().manual_seed(2)
    data = torch.rand((B,) + img, generator=gen)
    prior = torch.randn(B, D, generator=gen)
    p = {k: v.detach().cpu().double() for k, v in model.named_parameters()}
    mu, logvar = O.encoder_forward(p, data.double())
    recon = O.decoder_forward(p, mu)
    kl, _ = O.kl_normal_loss(mu, logvar)
    Rv = loss_f.weight * R.regulariser_torch(mu, prior.double(), kind, R.default_bandwidth(D))   # evaluation: z is the mean
    want = O.reconstruction_loss(data.double(), recon) + 0.75 * kl + Rv           # evaluation: no annealing
    calls = []
    real = _mmdlib.call
    _mmdlib.call = lambda name, *a: (calls.append((name, a)), real(name, *a))[1]
    try:
        storer = defaultdict(list)
        out = loss_f.fused_step(dev(data), model, None, storer, prior=dev(prior))
    finally:
        _mmdlib.call = real
    np.testing.assert_allclose(out.item(), want.item(), rtol=2e-5)
    z_dev = model.engine.buffers(B).z[:B].cpu().numpy()                          # the logged term: the restatement on the engine's own z
    ref = R.mmd(z_dev, prior.numpy(), kind, R.default_bandwidth(D), loss_f.weight)
    assert abs(storer["mmd_loss"][0] - ref["wmmd"]) <= R.tolerances(ref)["wmmd"]
    np.testing.assert_allclose(storer["mmd_loss"][0], Rv.item(), rtol=1e-3, atol=2e-5 * abs(want.item()))
    assert [name for name, _ in calls] == ["dvae_mmd_pairs", "dvae_mmd_finish"]
    assert calls[0][1][6] == 0 and calls[1][1][6] is None and calls[1][1][7] is None      # no gradient partials, no dmu, no dlv
    assert loss_f.n_train_steps == 0
    # without an injected prior an evaluation step draws one: the same seed, the same value; another seed, another value
    drawn = []
    for seed in (11, 11, 12):
        torch.manual_seed(seed)
        st = defaultdict(list)
        loss_f.fused_step(dev(data), model, None, st)
        drawn.append(st["mmd_loss"][0])
    assert drawn[0] == drawn[1] != drawn[2]

    class _Loader(list):
        pass
    ev = Evaluator(model, loss_f, device=torch.device(DEV), is_progress_bar=False)
    torch.manual_seed(11)
    losses = ev.compute_losses(_Loader([(data, None)]))
    assert list(losses) == list(storer) and losses["mmd_loss"] == drawn[0]


def _steps(img, D, B, replay=None, poisoned=False, n=3, inject=True, **info):
    """n seeded training steps -> (losses, parameters, gradients, loss object)."""
    model, opt, loss_f = _native(img, D, 33, 5e-4, **info)
    loss_f.replay = replay
    gen = torch.Generator().manual_seed(8)
    data = torch.empty((B,) + img, device=DEV)                                    # a plan is keyed on the batch's address
    losses = []
    torch.manual_seed(77)                                                         # the device generator, for the steps that draw
    for _ in range(n):
        data.copy_(torch.rand((B,) + img, generator=gen))
        eps = torch.randn(B, D, generator=gen).to(DEV) if inject else None
        prior = torch.randn(B, D, generator=gen).to(DEV) if inject else None
        if poisoned:
            paths = _poison(model, loss_f)
            assert any("mmd_dmu" in p for p in paths) or len(losses) == 0
        losses.append(loss_f.fused_step(data, model, opt, None, eps=eps, prior=prior).item())
    torch.cuda.synchronize()
    grads = torch.cat([model.arena.view(k, grad=True).reshape(-1) for k in model.arena.shapes])
    return losses, model.arena.flat.clone(), grads.clone(), loss_f


def _same(a, b, what):
    assert a[0] == b[0], "%s: losses %s vs %s" % (what, a[0], b[0])
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), what + ": parameters or gradients differ"


@pytest.mark.parametrize("inject", [True, False], ids=["injected", "drawn"])
@pytest.mark.parametrize("img,D,B,info", [((1, 32, 32), 10, 8, dict()), ((3, 64, 64), 10, 5, dict(mmd_kernel="rbf")),
                                          ((1, 32, 32), 20, 9, dict(info_alpha=1.0))])
def test_eager_plan_graph_and_auto_give_the_same_bits(img, D, B, info, inject):
    n = 6                                                                         # graph: the allocating step, two warm-up steps, the capture, two replays
    eager = _steps(img, D, B, None, n=n, inject=inject, **info)
    assert all(np.isfinite(eager[0]))
    for mode in ("plan", "graph", "auto"):
        got = _steps(img, D, B, mode, n=n, inject=inject, **info)
        _same(eager, got, "%s vs eager" % mode)
        if mode != "auto":
            assert got[3]._graphs.replays >= 2, "%s: the step was never replayed" % mode
    if inject:                                                                    # the prior reaches the replayed launches: another prior, other bits
        assert eager[0] != _steps(img, D, B, None, n=n, inject=False, **info)[0]


def test_the_hyper_parameters_join_the_replay_key():
    img, D, B = (1, 32, 32), 10, 8
    model, opt, loss_f = _native(img, D, 33, 5e-4)
    loss_f.replay = "plan"
    gen = torch.Generator().manual_seed(8)
    data = torch.rand((B,) + img, generator=gen).to(DEV)
    eps, prior = torch.randn(B, D, generator=gen).to(DEV), torch.randn(B, D, generator=gen).to(DEV)
    for _ in range(3):
        loss_f.fused_step(data, model, opt, None, eps=eps, prior=prior)
    replays = loss_f._graphs.replays
    assert replays >= 1
    for change in (dict(lam=3.0), dict(alpha=0.5), dict(kernel="rbf"), dict(bandwidth=11.0)):   # a recorded launch froze the old value
        for k, v in change.items():
            setattr(loss_f, k, v)
        storer = defaultdict(list)
        loss_f.n_train_steps = 50                                                 # the next step logs
        loss_f.fused_step(data, model, opt, storer, eps=eps, prior=prior)
        assert loss_f._graphs.replays == replays, change
        buf = model.engine.buffers(B)
        ref = R.mmd(buf.z[:B].cpu().numpy(), prior.cpu().numpy(), loss_f.kernel, loss_f._h(D), loss_f.weight)
        assert abs(storer["mmd_loss"][0] - ref["wmmd"]) <= R.tolerances(ref)["wmmd"], change


@pytest.mark.parametrize("img,D,B,info", [((1, 32, 32), 10, 8, dict()), ((1, 32, 32), 20, 9, dict(mmd_kernel="rbf"))])
def test_poisoned_buffers_change_no_bit(img, D, B, info):
    clean = _steps(img, D, B, **info)
    _same(clean, _steps(img, D, B, poisoned=True, **info), "poisoned engine buffers")
    _same(clean, _steps(img, D, B, "plan", poisoned=True, n=3, **info), "poisoned buffers under plan replay")


@pytest.mark.parametrize("kind", R.KERNELS)
def test_autograd_signature_gives_the_fused_steps_gradients(kind):
    """loss(data, recon, latent_dist, is_train, storer, latent_sample=z) through torch.autograd against fused_step on a twin: the
    bound of test_gpu_step.py::test_autograd_path_after_fused_step_does_not_double_gradients.  The autograd path draws its prior
    with one normal_() on a [B, D] device tensor: the same seed gives the twin the same draws."""
    img, B, D = (1, 64, 64), 6, 10
    m, o, l = _native(img, D, 7, 5e-4, mmd_kernel=kind)
    m2, o2, l2 = _native(img, D, 7, 5e-4, mmd_kernel=kind)
    gen = torch.Generator().manual_seed(3)
    data, eps = dev(torch.rand((B,) + img, generator=gen)), dev(torch.randn(B, D, generator=gen))
    recon, latent_dist, z = m(data, eps=eps)
    storer = defaultdict(list)
    torch.manual_seed(21)
    out = l(data, recon, latent_dist, True, storer, latent_sample=z)
    o.zero_grad(set_to_none=False)
    out.backward()
    torch.manual_seed(21)
    prior = torch.empty(B, D, device=DEV).normal_()
    storer2 = defaultdict(list)
    out2 = l2.fused_step(data, m2, o2, storer2, eps=eps, prior=prior)
    np.testing.assert_allclose(out.item(), out2.item(), rtol=2e-5)
    assert list(storer) == list(storer2)
    np.testing.assert_allclose(storer["mmd_loss"][0], storer2["mmd_loss"][0], rtol=2e-5, atol=2e-5 * abs(out2.item()))
    for (k, p), (_, p2) in zip(m.named_parameters(), m2.named_parameters()):
        check(p.grad, p2.grad, rtol=1e-5, atol_rel=4e-6, what="autograd path vs fused step " + k)
