"""-m gpu: the weakly-supervised pair losses Ada-GVAE / Ada-ML-VAE -- libdvae_weak_hip.so through its C-ABI against the fp64
restatement (tests/weak_ref.py), and whole training steps of WeakVaeLoss against the oracle.

Kernel level.  (P, D) in weak_ref.GPU_SIZES: one pair, D = 1 (no lane exchange), D on either side of a power of two (16 / 17: the
group of a pair grows from 16 to 32 lanes), a last workgroup that is not full, D = 64 (a whole wave per pair, bit 63 of the mask)
and 1024 pairs; both aggregations, both table families, and the edge table (ties, identical rows, log-variance differences of
+-40, -20 against +4).  Outside the band (weak_ref.band_of) the device's mask is the restatement's bit for bit; values, delta and
the backward pass are compared AT THE DEVICE'S MASK inside MARGIN = 4 times the first-order fp32 bounds of weak_ref (DESIGN.md
section 2); what is not shared is compared bit for bit.  Every case prints its worst error / bound at margin 1 before it asserts.

Whole step, shaped like test_gpu_dip.py::test_fused_step_vs_oracle, same tolerances: loss 2e-5; gradients rtol 1e-5 + 2e-6
max|g| against the gate-matched, mask-matched fp64 oracle (weak_ref.weak_iteration_grads fed the device's mask) at the engine's
parameters, three steps.
"""
import functools
from collections import defaultdict

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import weak_ref as R
from gpu_util import DEV, check, dev, stream
from guard_util import Guarded, run_contract
from oracle import disvae_oracle as O
from oracle.gate_match import engine_gates, gate_mismatches
from disvae_amd import _lib, _weaklib, engine as ENGINE
from disvae_amd import schedule as SCHED
from disvae_amd.data import PairedFactorLoader
from disvae_amd.evaluate import Evaluator
from disvae_amd.models import losses as L
from disvae_amd.models.losses import adaptive_group_posterior, get_loss_f
from disvae_amd.models.vae import init_specific_model
from disvae_amd.training import Trainer
from test_gpu_step_poison import _poison


@functools.lru_cache(maxsize=None)
def _reference(family, P, D):
    """(mu, lv, band, own mask, gradients to push back): computed once, shared by the tests, never written to."""
    mu, lv = R.table(family, P, D)
    rng = np.random.RandomState(P + 31 * D)
    g = rng.randn(2 * P, 2 * D).astype(np.float32)
    return mu, lv, R.band_of(mu, lv), R.aggregate(mu, lv, "gvae")["own"], g


def _fwd(mu, lv, kind, want_delta=True):
    """The forward launch on device copies -> (ml_agg [2 P, 2 D], mask words int64 [P], delta [P, D] or None) as numpy."""
    B, D = mu.shape
    ml = torch.tensor(R.interleave(mu, lv), device=DEV)
    ml_agg = torch.full((B, 2 * D), float("nan"), device=DEV)
    shared = torch.full((B // 2,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=DEV)
    delta = torch.full((B // 2, D), float("nan"), device=DEV) if want_delta else None
    _weaklib.call("dvae_weak_aggregate_fwd", ml.data_ptr(), B // 2, D, _weaklib.KINDS[kind], ml_agg.data_ptr(), shared.data_ptr(),
                  None if delta is None else delta.data_ptr(), stream())
    torch.cuda.synchronize()
    return ml_agg.cpu().numpy(), shared.cpu().numpy(), None if delta is None else delta.cpu().numpy()


def _bwd(mu, lv, words, kind, g):
    """The backward launch: g [2 P, 2 D] (gradient with respect to ml_agg) -> the gradient with respect to ml."""
    B, D = mu.shape
    ml = torch.tensor(R.interleave(mu, lv), device=DEV)
    shared = torch.tensor(words, dtype=torch.int64, device=DEV)
    dml = torch.tensor(g, device=DEV)
    _weaklib.call("dvae_weak_aggregate_bwd", ml.data_ptr(), shared.data_ptr(), B // 2, D, _weaklib.KINDS[kind], dml.data_ptr(), stream())
    torch.cuda.synchronize()
    return dml.cpu().numpy()


def _check_case(mu, lv, g, kind, what, worst, band=None, own=None):
    """One table through both launches against the restatement at the device's mask; updates `worst` (error / bound, margin 1)."""
    B, D = mu.shape
    P = B // 2
    ml_agg, words, delta = _fwd(mu, lv, kind)
    assert np.isfinite(ml_agg).all() and np.isfinite(delta).all(), what
    if D < 64:
        assert not (words.view(np.uint64) >> np.uint64(D)).any(), what + ": mask bits at or above D"
    sh = R.unbits(words, D)
    if band is not None:
        assert np.array_equal(sh[~band], own[~band]), what + ": the mask differs from the restatement's outside the band"
    ref = R.aggregate(mu, lv, kind, shared=sh)
    fb = R.forward_bounds(mu, lv, kind)
    err = np.abs(delta - ref["delta"]) / fb["delta"]
    worst["delta"] = max(worst["delta"], float(err.max()))
    assert err.max() <= R.MARGIN, what + ": delta %.3g x the bound" % err.max()
    got_mu, got_lv = ml_agg[:, 0::2], ml_agg[:, 1::2]
    sh2 = np.concatenate([sh, sh])
    # what is not shared is a copy; a shared element holds the same bits in both rows
    assert got_mu[~sh2].tobytes() == mu[~sh2].tobytes() and got_lv[~sh2].tobytes() == lv[~sh2].tobytes(), what + ": a kept element changed"
    assert got_mu[:P][sh].tobytes() == got_mu[P:][sh].tobytes() and got_lv[:P][sh].tobytes() == got_lv[P:][sh].tobytes(), what
    if sh.any():
        em = (np.abs(got_mu[:P] - ref["mu"][:P]) / fb["m"])[sh].max()
        el = (np.abs(got_lv[:P] - ref["lv"][:P]) / fb["lvt"])[sh].max()
        worst["m"], worst["lvt"] = max(worst["m"], float(em)), max(worst["lvt"], float(el))
        assert em <= R.MARGIN and el <= R.MARGIN, what + ": m %.3g, lv~ %.3g x the bound" % (em, el)
    # backward against fp64 autograd of the torch restatement at the device's mask
    dml = _bwd(mu, lv, words, kind, g)
    gm, gl = g[:, 0::2], g[:, 1::2]
    tmu = torch.tensor(mu, dtype=torch.float64, requires_grad=True)
    tlv = torch.tensor(lv, dtype=torch.float64, requires_grad=True)
    am, al = R.aggregate_torch(tmu, tlv, kind, sh)
    rmu, rlv = torch.autograd.grad((am * torch.tensor(gm, dtype=torch.float64)).sum() + (al * torch.tensor(gl, dtype=torch.float64)).sum(),
                                   [tmu, tlv])
    e_mu, e_lv = R.backward_bounds(mu, lv, gm, gl, kind)
    dmu, dlv = dml[:, 0::2], dml[:, 1::2]
    assert np.isfinite(dml).all(), what
    assert dmu[~sh2].tobytes() == gm[~sh2].tobytes() and dlv[~sh2].tobytes() == gl[~sh2].tobytes(), what + ": a kept gradient changed"
    if sh.any():
        bm = (np.abs(dmu - rmu.numpy()) / e_mu)[sh2].max()
        bl = (np.abs(dlv - rlv.numpy()) / e_lv)[sh2].max()
        worst["dmu"], worst["dlv"] = max(worst["dmu"], float(bm)), max(worst["dlv"], float(bl))
        assert bm <= R.MARGIN and bl <= R.MARGIN, what + ": dmu %.3g, dlv %.3g x the bound" % (bm, bl)
    return words


def _worst():
    return dict(delta=0.0, m=0.0, lvt=0.0, dmu=0.0, dlv=0.0)


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_kernels_against_the_restatement(family, kind):
    worst = _worst()
    for P, D in R.GPU_SIZES:
        mu, lv, band, own, g = _reference(family, P, D)
        what = "%s %s P=%d D=%d" % (family, kind, P, D)
        if D == 1:                                                         # delta = tau: nothing can be shared
            words = _check_case(mu, lv, g, kind, what, worst)
            assert not words.any(), what
            continue
        assert band.mean() <= 0.005 and not band.any(), what + ": %d entries in the band" % band.sum()
        words = _check_case(mu, lv, g, kind, what, worst, band, own)
        assert words.view(np.uint64).tolist() == R.bits_of(own).tolist(), what
    print("%s %s: worst error / bound at margin 1 -- delta %.3g, m %.3g, lv~ %.3g, dmu %.3g, dlv %.3g (allowed: %g)"
          % (family, kind, worst["delta"], worst["m"], worst["lvt"], worst["dmu"], worst["dlv"], R.MARGIN))


@pytest.mark.parametrize("kind", R.KINDS)
def test_ties_identical_rows_and_extreme_log_variances(kind):
    worst = _worst()
    for D in (1, 2, 10, 17, 64):
        mu, lv, expected = R.edge_table(D)
        g = np.random.RandomState(D).randn(mu.shape[0], 2 * D).astype(np.float32)
        band, own = R.band_of(mu, lv), R.aggregate(mu, lv, kind)["own"]
        band[:3] = True                                                    # pairs 0 .. 2: ties, the mask is fixed by construction instead
        words = _check_case(mu, lv, g, kind, "edge %s D=%d" % (kind, D), worst, band, own)
        for i, want in enumerate(expected):
            if want is not None:
                assert words.view(np.uint64)[i] == want, (D, i, hex(int(words.view(np.uint64)[i])))
        if D > 1:
            assert words[3] != 0 and words[4] != 0 and words[5] != 0       # the extreme pairs do share something
    print("edge %s: worst error / bound at margin 1 -- delta %.3g, m %.3g, lv~ %.3g, dmu %.3g, dlv %.3g (allowed: %g)"
          % (kind, worst["delta"], worst["m"], worst["lvt"], worst["dmu"], worst["dlv"], R.MARGIN))


def test_two_runs_give_the_same_bytes_and_delta_is_optional():
    for kind in R.KINDS:
        for P, D in ((3, 10), (257, 17), (5, 64), (1024, 10)):
            mu, lv, _, _, g = _reference("regime", P, D)
            a, b = _fwd(mu, lv, kind), _fwd(mu, lv, kind)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), (kind, P, D)
            c = _fwd(mu, lv, kind, want_delta=False)
            assert c[2] is None and c[0].tobytes() == a[0].tobytes() and c[1].tobytes() == a[1].tobytes()
            assert _bwd(mu, lv, a[1], kind, g).tobytes() == _bwd(mu, lv, a[1], kind, g).tobytes()


def test_a_latent_dimension_above_the_limit_is_refused_without_a_launch():
    t = torch.zeros(4 * 2 * 65, device=DEV)
    out = torch.full((4 * 2 * 65,), 7.0, device=DEV)
    w = torch.full((2,), 7, dtype=torch.int64, device=DEV)
    for name, args in (("dvae_weak_aggregate_fwd", (t.data_ptr(), 2, 65, 0, out.data_ptr(), w.data_ptr(), None, stream())),
                       ("dvae_weak_aggregate_bwd", (t.data_ptr(), w.data_ptr(), 2, 65, 0, out.data_ptr(), stream()))):
        with pytest.raises(_lib.DvaeHipError, match="invalid argument.*DVAE_WEAK_MAX_D"):
            _weaklib.call(name, *args)
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (w == 7).all()
    with pytest.raises(ValueError):
        adaptive_group_posterior(torch.zeros(4, 65, device=DEV), torch.zeros(4, 65, device=DEV))


def _weak_call(name):
    return lambda args: _weaklib.call(name, *[a.ptr if isinstance(a, Guarded) else a for a in args])


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("P,D", [(1, 1), (3, 10), (65, 16), (33, 20), (5, 64)])
def test_memory_contract(P, D, kind):
    """Guard-banded, NaN-poisoned buffers at 256-byte alignment and at the weakest the header promises (8 bytes for the couples
    and the mask words, 4 for delta): guards untouched, inputs unchanged, every defined output written, the same bits in all runs."""
    mu, lv, _, _, g = _reference("gauss", P, D)
    ml = R.interleave(mu, lv)
    k = _weaklib.KINDS[kind]

    def fwd(al):
        return [al.inp("ml", ml, align=8), P, D, k, al.out("ml_agg", (2 * P, 2 * D), align=8),
                al.out("shared", (P,), dtype=torch.int64, align=8), al.out("delta", (P, D), align=4), stream()]
    runs = run_contract("dvae_weak_aggregate_fwd", fwd, fn=_weak_call("dvae_weak_aggregate_fwd"))
    got = {a.name: a.t.cpu().numpy() for a in runs[2].args}
    plain = _fwd(mu, lv, kind)
    assert got["ml_agg"].tobytes() == plain[0].tobytes() and got["shared"].tobytes() == plain[1].tobytes()
    assert got["delta"].tobytes() == plain[2].tobytes()

    def bwd(al):
        return [al.inp("ml", ml, align=8), al.inp("shared", torch.tensor(plain[1]), align=8), P, D, k, al.inout("dml", g, align=8), stream()]
    runs = run_contract("dvae_weak_aggregate_bwd", bwd, fn=_weak_call("dvae_weak_aggregate_bwd"))
    assert runs[2].args[2].t.cpu().numpy().tobytes() == _bwd(mu, lv, plain[1], kind, g).tobytes()


@pytest.mark.parametrize("kind", R.KINDS)
def test_adaptive_group_posterior_is_the_two_launches_under_autograd(kind):
    P, D = 33, 10
    mu, lv, band, own, g = _reference("gauss", P, D)
    tmu = torch.tensor(mu, device=DEV, requires_grad=True)
    tlv = torch.tensor(lv, device=DEV, requires_grad=True)
    am, al, shared = adaptive_group_posterior(tmu, tlv, kind)
    assert shared.dtype == torch.int64 and not shared.requires_grad and am.requires_grad
    ml_agg, words, _ = _fwd(mu, lv, kind)
    assert shared.cpu().numpy().tobytes() == words.tobytes()
    assert am.detach().cpu().numpy().tobytes() == ml_agg[:, 0::2].tobytes() and al.detach().cpu().numpy().tobytes() == ml_agg[:, 1::2].tobytes()
    gm, gl = torch.tensor(g[:, 0::2].copy(), device=DEV), torch.tensor(g[:, 1::2].copy(), device=DEV)
    dmu, dlv = torch.autograd.grad((am * gm).sum() + (al * gl).sum(), [tmu, tlv])
    dml = _bwd(mu, lv, words, kind, g)
    assert dmu.cpu().numpy().tobytes() == dml[:, 0::2].tobytes() and dlv.cpu().numpy().tobytes() == dml[:, 1::2].tobytes()
    (only_mu,) = torch.autograd.grad(adaptive_group_posterior(tmu, tlv, kind)[0].sum(), [tmu])      # a missing gradient is zero
    assert torch.isfinite(only_mu).all()


# ---- whole steps ------------------------------------------------------------------------------------------------------------------
HP = dict(rec_dist="bernoulli", reg_anneal=10000, betaH_B=4, betaB_initC=0, betaB_finC=25, betaB_G=1000, factor_G=6.4,
          lr_disc=1e-4, btcvae_A=1, btcvae_B=6.4, btcvae_G=1, n_data=202599)
G_RTOL, G_ATOL = 1e-5, 2e-6
AGG = {"adagvae": "gvae", "adamlvae": "mlvae"}
STEP_CASES = [("adagvae", (1, 32, 32), 4, 10, "bernoulli"), ("adamlvae", (3, 64, 64), 3, 10, "gaussian"),
              ("adagvae", (1, 64, 64), 17, 10, "bernoulli"), ("adamlvae", (1, 32, 32), 1, 10, "bernoulli"),
              ("adagvae", (1, 32, 32), 5, 20, "bernoulli")]


def _native(loss, img, D, seed, lr, rec_dist="bernoulli"):
    torch.manual_seed(seed)
    model = init_specific_model("Burgess", img, D)
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    loss_f = get_loss_f(loss, device=torch.device(DEV), latent_dim=D, **dict(HP, rec_dist=rec_dist))
    model.to(DEV)
    model.train()
    return model, opt, loss_f


def _device_mask(loss_f, D):
    return R.unbits(loss_f._shared.cpu().numpy(), D)


@pytest.mark.parametrize("loss,img,P,D,rec_dist", STEP_CASES)
def test_fused_step_vs_oracle(loss, img, P, D, rec_dist):
    seed, lr, B = 1234, 5e-4, 2 * P
    model, opt, loss_f = _native(loss, img, D, seed, lr, rec_dist)
    hp = dict(HP, latent_dim=D)
    gen = torch.Generator().manual_seed(seed + 1)
    for step in range(3):
        data = torch.rand((B,) + tuple(img), generator=gen)               # independent random images per row
        eps = torch.randn(B, D, generator=gen)
        p_step = {k: p.detach().cpu().clone() for k, p in model.named_parameters()}
        storer = defaultdict(list)
        out = loss_f.fused_step(dev(data), model, opt, storer, eps=dev(eps))
        buf = model.engine.buffers(B)
        sh = _device_mask(loss_f, D)
        st = O.LossState(rec_dist=rec_dist, steps_anneal=HP["reg_anneal"]); st.n_train_steps = step
        ref_loss, ref_logs, _, ref_outs = R.weak_iteration_grads(AGG[loss], hp, st, O.clone_params(p_step, requires_grad=True), data, eps,
                                                                 shared=sh)
        print("%s step %d: loss %.6f (oracle %.6f), %.2f shared dimensions per pair" % (loss, step, out.item(), ref_loss.item(), sh.sum(1).mean()))
        np.testing.assert_allclose(out.item(), ref_loss.item(), rtol=2e-5, err_msg="loss step %d" % step)
        check(buf.mu, ref_outs["mu"], what="mu")
        check(buf.logvar, ref_outs["logvar"], what="logvar")
        check(buf.recon, ref_outs["recon"], what="recon")
        gates = engine_gates(model, B)
        log = []
        p64 = O.clone_params(p_step, dtype=torch.float64)
        with torch.no_grad(), O.gates(None, record=log):
            _, _, _, outs64 = R.weak_iteration_grads(AGG[loss], hp, O.LossState(rec_dist=rec_dist), p64, data.double(), eps.double(),
                                                     shared=sh, is_train=False)
        n_diff, gate_worst, ok = gate_mismatches(gates, log)
        assert ok, "a ReLU gated differently than in fp64 at |pre-activation| = %.2e of the layer scale" % gate_worst
        # outside the band the device's mask is the fp64 oracle's own
        mu0, lv0 = outs64["mu0"].numpy(), outs64["logvar0"].numpy()
        band, own = R.band_of(mu0, lv0), R.aggregate(mu0, lv0, "gvae")["own"]
        assert np.array_equal(sh[~band], own[~band]), "step %d: %d mask bits differ outside the band" % (step, (sh != own)[~band].sum())
        st64 = O.LossState(rec_dist=rec_dist, steps_anneal=HP["reg_anneal"]); st64.n_train_steps = step
        with O.gates(gates):
            _, _, grads64, _ = R.weak_iteration_grads(AGG[loss], hp, st64, O.clone_params(p_step, dtype=torch.float64, requires_grad=True),
                                                      data.double(), eps.double(), shared=sh)
        for k, p in model.named_parameters():
            check(p.grad, grads64[k], rtol=G_RTOL, atol_rel=G_ATOL, what="%s step %d grad vs gate-matched fp64 %s" % (loss, step, k))
        if step == 0:
            assert list(storer.keys()) == list(ref_logs.keys()), (list(storer.keys()), list(ref_logs.keys()))
            for k in ref_logs:
                np.testing.assert_allclose(storer[k][0], ref_logs[k].item(), rtol=5e-5, atol=1e-6, err_msg=k)
            assert 0 <= storer["shared_dims"][0] < D
        else:
            assert len(storer) == 0
    assert loss_f.n_train_steps == 3


def _poison_all(model, loss_f):
    paths = _poison(model, loss_f)
    for ml_agg, shared, delta in loss_f._weak.values():
        ml_agg.fill_(float("nan")); delta.fill_(float("nan")); shared.fill_(0x5A5A5A5A5A5A5A5A)
    torch.cuda.synchronize()
    return paths


def _steps(loss, img, D, P, replay=None, poisoned=False, single=False, n=3):
    """n seeded training steps -> (losses, parameters, gradients, Adam moments, loss object)."""
    B = 2 * P
    model, opt, loss_f = _native(loss, img, D, 33, 5e-4)
    loss_f.replay = replay
    if single:
        sw = tuple("1" if name == "DVAE_STREAMS" else v for (name, _), v in zip(SCHED.SWITCHES, SCHED.switches()))
        pol = SCHED.build_policy(tuple(img), D, B, sw, 1, loss_f.KIND, True, None)
        assert pol.single_stream
        loss_f.policy_override = pol._asdict()
    gen = torch.Generator().manual_seed(8)
    data = torch.empty((B,) + img, device=DEV)                            # a plan is keyed on the batch's address
    losses = []
    for _ in range(n):
        data.copy_(torch.rand((B,) + img, generator=gen))
        eps = torch.randn(B, D, generator=gen).to(DEV)
        if poisoned:
            _poison_all(model, loss_f)
        losses.append(loss_f.fused_step(data, model, opt, None, eps=eps).item())
    torch.cuda.synchronize()
    assert not model.engine.policy.fuse_ends
    grads = torch.cat([model.arena.view(k, grad=True).reshape(-1) for k in model.arena.shapes])
    moments = torch.cat([opt.state[p][k].reshape(-1) for p in model.parameters() for k in ("exp_avg", "exp_avg_sq")])
    return losses, model.arena.flat.clone(), grads.clone(), moments.clone(), loss_f


def _same(a, b, what):
    assert a[0] == b[0], "%s: losses %s vs %s" % (what, a[0], b[0])
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]), what + ": parameters, gradients or Adam moments differ"


@pytest.mark.parametrize("loss,img,D,P", [("adagvae", (1, 32, 32), 10, 4), ("adamlvae", (3, 64, 64), 10, 3), ("adagvae", (1, 32, 32), 20, 5)])
def test_eager_plan_graph_and_auto_give_the_same_bits(loss, img, D, P):
    n = 6                                                                 # graph: the allocating step, two warm-up steps, the capture, two replays
    eager = _steps(loss, img, D, P, None, n=n)
    assert all(np.isfinite(eager[0]))
    for mode in ("plan", "graph", "auto"):
        got = _steps(loss, img, D, P, mode, n=n)
        _same(eager, got, "%s vs eager" % mode)
        if mode != "auto":
            assert got[4]._graphs.replays >= 2, "%s: the step was never replayed" % mode


@pytest.mark.parametrize("loss,img,D,P", [("adagvae", (1, 32, 32), 10, 4), ("adamlvae", (1, 64, 64), 20, 3)])
def test_poisoned_buffers_and_the_single_stream_policy_change_no_bit(loss, img, D, P):
    clean = _steps(loss, img, D, P)
    _same(clean, _steps(loss, img, D, P, poisoned=True), "poisoned engine buffers")
    _same(clean, _steps(loss, img, D, P, single=True), "single-stream policy")
    _same(clean, _steps(loss, img, D, P, "plan", poisoned=True, n=3), "poisoned buffers under plan replay")


@pytest.mark.parametrize("loss", L.WEAK_LOSSES)
def test_eval_mode_computes_the_value_only(loss, monkeypatch):
    img, P, D = (1, 32, 32), 3, 10
    model, opt, loss_f = _native(loss, img, D, 5, 5e-4)
    model.eval()
    gen = torch.Generator().manual_seed(2)
    data = torch.rand((2 * P,) + img, generator=gen)
    names = []
    for mod in (ENGINE, L):
        real = mod.call
        monkeypatch.setattr(mod, "call", lambda name, *a, _real=real: (names.append(name), _real(name, *a))[1])
    real_weak = _weaklib.call
    monkeypatch.setattr(_weaklib, "call", lambda name, *a: (names.append(name), real_weak(name, *a))[1])
    rng = torch.cuda.get_rng_state()
    storer = defaultdict(list)
    out = loss_f.fused_step(dev(data), model, None, storer)
    assert torch.equal(torch.cuda.get_rng_state(), rng), "an evaluation step drew noise"
    assert names.count("dvae_weak_aggregate_fwd") == 1 and names.count("dvae_linear_fwd") == 6 and "dvae_loss_epilogue" in names
    assert not [n for n in names if "bwd" in n or "dgrad" in n or "wgrad" in n or "fc_chain" in n], names
    sh = _device_mask(loss_f, D)
    p = {k: v.detach().cpu().double() for k, v in model.named_parameters()}
    want, logs, _, outs = R.weak_iteration_grads(AGG[loss], dict(HP, latent_dim=D), O.LossState(), p, data.double(), None, shared=sh,
                                                 is_train=False)
    np.testing.assert_allclose(out.item(), want.item(), rtol=2e-5)
    check(model.engine.buffers(2 * P).z, outs["mu"], what="z = m~ in evaluation")
    assert list(storer) == list(logs) and loss_f.n_train_steps == 0
    np.testing.assert_allclose(storer["shared_dims"][0], sh.sum(1).mean())


@pytest.mark.parametrize("loss", L.WEAK_LOSSES)
def test_identical_pairs_are_a_plain_vae_step(loss):
    img, P, D = (1, 32, 32), 4, 10
    gen = torch.Generator().manual_seed(4)
    half = torch.rand((P,) + img, generator=gen)
    data, eps = dev(torch.cat([half, half])), dev(torch.randn(2 * P, D, generator=gen))
    model, opt, loss_f = _native(loss, img, D, 9, 5e-4)
    storer = defaultdict(list)
    out = loss_f.fused_step(data, model, opt, storer, eps=eps)
    vae_model, vae_opt, vae_f = _native("VAE", img, D, 9, 5e-4)
    want = vae_f.fused_step(data, vae_model, vae_opt, None, eps=eps)
    print("%s on identical pairs: loss %.6f, VAE %.6f, shared_dims %g" % (loss, out.item(), want.item(), storer["shared_dims"][0]))
    np.testing.assert_allclose(out.item(), want.item(), rtol=2e-5)
    assert storer["shared_dims"][0] == 0


def test_trainer_and_evaluator_on_a_paired_loader(tmp_path):
    sizes, img, P, D = (3, 4, 2), (1, 32, 32), 4, 10
    images = torch.randint(0, 256, (24,) + img, dtype=torch.uint8, generator=torch.Generator().manual_seed(1))
    loader = PairedFactorLoader(images, sizes, batch_size=P, k=1, device=DEV)
    assert len(loader) == 6
    model, opt, loss_f = _native("adagvae", img, D, 3, 5e-4)
    trainer = Trainer(model, opt, loss_f, device=torch.device(DEV), save_dir=str(tmp_path), is_progress_bar=False)
    torch.manual_seed(0)
    trainer(loader, epochs=2, checkpoint_every=10)
    assert loss_f.n_train_steps == 12
    logged = open(tmp_path / "train_losses.log").read().splitlines()
    keys = [line.split(",")[1] for line in logged[1:]]
    assert keys == ["recon_loss", "kl_loss"] + ["kl_loss_%d" % i for i in range(D)] + ["shared_dims", "loss"]
    values = {line.split(",")[1]: float(line.split(",")[2]) for line in logged[1:]}
    assert all(np.isfinite(v) for v in values.values()) and 0 <= values["shared_dims"] < D
    ev = Evaluator(model, loss_f, device=torch.device(DEV), is_progress_bar=False)
    losses = ev.compute_losses(loader)
    assert list(losses) == keys and all(np.isfinite(v) for v in losses.values()) and 0 <= losses["shared_dims"] < D
    assert loss_f.n_train_steps == 12
