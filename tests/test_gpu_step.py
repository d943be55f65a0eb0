"""-m gpu: whole training iterations of the native engine (through the C-ABI) vs the oracle
and vs the golden vectors recorded from the real reference, same seeds / weights / noise.

Stated fp32 tolerances (north_star: "within a stated fp32 tolerance"):
  FIRST step (identical weights on both sides):
    loss scalars rtol 2e-5 | activations rtol 1e-4 (+2e-5 max) | gradients rtol 1e-5 (+2e-6 max|g|), NO outliers, against
    the fp64 oracle evaluated with the engine's ReLU on/off pattern (oracle/gate_match.py: a unit whose pre-activation is
    within fp32 rounding of 0 is gated differently by ANY two arithmetics -- the fp32 and fp64 oracles differ from each
    other by 1e-5 .. 3e-4 of max|g| for that reason); the pattern itself is checked: units gated differently than in fp64
    must sit within 1e-5 of the layer scale of zero -- the same bar as tests/test_gpu_bench_sizes.py;
    parameters after the Adam step: atol 2.5*lr (Adam's first update is lr*sign(g): a gradient
    entry that is ~0 up to rounding may move by 2*lr in opposite directions).
  LATER steps (each side follows its own trajectory; Adam's normalisation amplifies the above):
    loss rtol 1e-3, gradients rtol 2e-2 (+5e-3 max|g|), <= 2 % outliers."""
from collections import defaultdict

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import *  # noqa
from gpu_util import _lib  # noqa
from golden_util import load, tensor_digest, assert_digest_close
from oracle import disvae_oracle as O
from oracle.gate_match import engine_gates, discriminator_gates, gate_mismatches
from disvae_amd.models.vae import init_specific_model
from disvae_amd.models.losses import get_loss_f
from disvae_amd.training import Trainer

HP = dict(rec_dist="bernoulli", reg_anneal=10000, betaH_B=4, betaB_initC=0, betaB_finC=25,
          betaB_G=1000, factor_G=6.4, latent_dim=10, lr_disc=1e-4, btcvae_A=1, btcvae_B=6.4,
          btcvae_G=1)


def _native(loss, img, seed, n_data, lr, rec_dist="bernoulli"):
    torch.manual_seed(seed)
    model = init_specific_model("Burgess", img, 10)
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    hp = dict(HP, rec_dist=rec_dist)
    loss_f = get_loss_f(loss, n_data=n_data, device=torch.device(DEV), **hp)
    model.to(DEV)
    model.train()
    return model, opt, loss_f


G_RTOL, G_ATOL = 1e-5, 2e-6        # gradients of EVERY step vs the gate-matched fp64 oracle at the engine's parameters, no outliers


def _assert_gate_pattern(gates, log, what):
    n_diff, worst, ok = gate_mismatches(gates, log)
    assert ok, "%s: a ReLU gated differently than in fp64 at |pre-activation| = %.2e of the layer scale" % (what, worst)


@pytest.mark.parametrize("loss,img,B,rec_dist", [
    ("VAE", (1, 32, 32), 8, "bernoulli"), ("betaB", (1, 32, 32), 8, "bernoulli"),
    ("betaH", (3, 64, 64), 5, "gaussian"), ("betaH", (1, 64, 64), 4, "laplace"),
    ("btcvae", (1, 64, 64), 16, "bernoulli"), ("btcvae", (3, 64, 64), 12, "bernoulli"),
    ("btcvae", (3, 64, 64), 70, "bernoulli"),
    # ragged / minimal batches (below one MFMA tile, odd, straddling a 32-row tile)
    ("btcvae", (3, 64, 64), 3, "bernoulli"), ("btcvae", (1, 64, 64), 33, "bernoulli"),
    ("btcvae", (3, 64, 64), 2, "bernoulli"), ("VAE", (3, 32, 32), 7, "bernoulli"),
])
def test_fused_step_vs_oracle(loss, img, B, rec_dist):
    seed, n_data, lr = 1234, 202599, 5e-4
    model, opt, loss_f = _native(loss, img, seed, n_data, lr, rec_dist)
    torch.manual_seed(seed)
    params = O.init_vae_params(img, 10)
    hp = dict(HP, n_data=n_data)
    # Every step is checked the way the first one is: the oracle is evaluated AT THE ENGINE'S CURRENT PARAMETERS (fp32 for the
    # loss / outputs / logged scalars, gate-matched fp64 for the gradients, rtol 1e-5, no outliers), so steps 2 and 3 hold the
    # arena reuse, the cached gradient views, the advancing annealing coefficient and the weights Adam has moved to the same
    # bound.  The optimizer is checked on its own: torch's CPU Adam fed with the engine's gradients must land on the engine's
    # parameters (<= 2 ulp, or 4e-6 of an update).
    cpu = [p.detach().cpu().clone().requires_grad_(True) for p in model.parameters()]
    oc = torch.optim.Adam(cpu, lr=lr)
    assert all(torch.equal(pc.detach(), params[k]) for pc, (k, _) in zip(cpu, model.named_parameters()))
    gen = torch.Generator().manual_seed(seed + 1)
    for step in range(3):
        data = torch.rand((B,) + tuple(img), generator=gen)
        eps = torch.randn(B, 10, generator=gen)
        p_step = {k: p.detach().cpu().clone() for k, p in model.named_parameters()}
        st = O.LossState(rec_dist=rec_dist, steps_anneal=HP["reg_anneal"]); st.n_train_steps = step
        ref_loss, ref_logs, _, ref_outs = O.train_iteration_grads(loss, hp, st, O.clone_params(p_step, requires_grad=True),
                                                                  data, eps)
        storer = defaultdict(list)
        out = loss_f.fused_step(dev(data), model, opt, storer, eps=dev(eps))
        buf = model.engine.buffers(B)
        np.testing.assert_allclose(out.item(), ref_loss.item(), rtol=2e-5, err_msg="loss step %d" % step)
        check(buf.mu, ref_outs["mu"], what="mu")
        check(buf.logvar, ref_outs["logvar"], what="logvar")
        check(buf.z, ref_outs["z"], what="z")
        check(buf.recon, ref_outs["recon"], what="recon")
        # gradient reference = the fp64 oracle evaluated with the engine's ReLU on/off pattern; the pattern is checked
        gates = engine_gates(model, B)
        log = []
        with torch.no_grad(), O.gates(None, record=log):
            O.vae_forward(O.clone_params(p_step, dtype=torch.float64), data.double(), eps.double())
        _assert_gate_pattern(gates, log, "%s B=%d step %d" % (loss, B, step))
        st64 = O.LossState(rec_dist=rec_dist, steps_anneal=HP["reg_anneal"]); st64.n_train_steps = step
        with O.gates(gates):
            _, _, grads64, _ = O.train_iteration_grads(loss, hp, st64, O.clone_params(p_step, dtype=torch.float64,
                                                                                     requires_grad=True),
                                                       data.double(), eps.double())
        for k, p in model.named_parameters():
            check(p.grad, grads64[k], rtol=G_RTOL, atol_rel=G_ATOL, what="%s step %d grad vs gate-matched fp64 %s" % (loss, step, k))
        if step == 0:
            assert list(storer.keys()) == list(ref_logs.keys()), (list(storer.keys()), list(ref_logs.keys()))
            for k in ref_logs:
                np.testing.assert_allclose(storer[k][0], ref_logs[k].item(), rtol=5e-5, atol=1e-6, err_msg=k)
        else:
            assert len(storer) == 0
        for pc, (k, p) in zip(cpu, model.named_parameters()):
            pc.grad = p.grad.detach().cpu().clone()
        oc.step()
        for pc, (k, p) in zip(cpu, model.named_parameters()):
            d = (p.detach().cpu() - pc.detach()).abs()
            tol = 2 * pc.detach().abs() * 2.0 ** -23 + 4e-6 * lr
            assert bool((d <= tol).all()), "param %s after step %d: GPU Adam vs torch CPU Adam on the same gradients: max diff %.3e" % (k, step, d.max().item())
    assert loss_f.n_train_steps == 3


@pytest.mark.parametrize("img,B", [((1, 64, 64), 8), ((3, 64, 64), 20), ((1, 32, 32), 6), ((3, 64, 64), 6), ((1, 64, 64), 2)])
def test_factor_step_vs_oracle(img, B):
    seed, n_data, lr = 1234, 737280, 1e-4
    model, opt, loss_f = _native("factor", img, seed, n_data, lr)
    torch.manual_seed(seed)
    params = O.init_vae_params(img, 10)
    dparams = O.init_disc_params(10)
    for k, v in loss_f.discriminator.state_dict().items():
        assert torch.equal(v.cpu(), dparams[k]), k
    hp = dict(HP, n_data=n_data)
    # every step at the engine's CURRENT parameters (see test_fused_step_vs_oracle): gate-matched fp64 gradients at 1e-5 for
    # the VAE and the discriminator, both optimizers against torch's CPU Adam on the engine's gradients
    cpu = [p.detach().cpu().clone().requires_grad_(True) for p in model.parameters()]
    dcpu = [p.detach().cpu().clone().requires_grad_(True) for p in loss_f.discriminator.parameters()]
    oc = torch.optim.Adam(cpu, lr=lr)
    ocd = torch.optim.Adam(dcpu, lr=HP["lr_disc"], betas=(0.5, 0.9))
    gen = torch.Generator().manual_seed(seed + 1)
    Bh = B // 2
    for step in range(3):
        data = torch.rand((B,) + tuple(img), generator=gen)
        eps1, eps2 = torch.randn(Bh, 10, generator=gen), torch.randn(Bh, 10, generator=gen)
        perms = torch.stack([torch.randperm(Bh, generator=gen) for _ in range(10)])
        p_step = {k: p.detach().cpu().clone() for k, p in model.named_parameters()}
        d_step = {k: p.detach().cpu().clone() for k, p in loss_f.discriminator.named_parameters()}
        st = O.LossState(steps_anneal=HP["reg_anneal"]); st.n_train_steps = step
        ref_loss, ref_logs, _, _, outs = O.factor_iteration_grads(hp, st, O.clone_params(p_step, requires_grad=True),
                                                                  O.clone_params(d_step, requires_grad=True), data, eps1, eps2,
                                                                  list(perms))
        storer = defaultdict(list)
        out = loss_f.call_optimize(dev(data), model, opt, storer, noise=(dev(eps1), dev(eps2), perms))
        np.testing.assert_allclose(out.item(), ref_loss.item(), rtol=2e-5)
        buf = model.engine.buffers(B)
        check(buf.z[:Bh], outs["z1"], what="z1")
        check(buf.z[Bh:2 * Bh], outs["z2"], what="z2")
        gates = engine_gates(model, B, splits=[slice(0, Bh), slice(Bh, 2 * Bh)], dec_rows=slice(0, Bh))
        gates.update(discriminator_gates(loss_f.discriminator, 2 * Bh, Bh))
        c64 = lambda p_: O.clone_params(p_, dtype=torch.float64, requires_grad=True)

        def args64():
            st64 = O.LossState(steps_anneal=HP["reg_anneal"]); st64.n_train_steps = step
            return (hp, st64, c64(p_step), c64(d_step), data.double(), eps1.double(), eps2.double(), list(perms))
        log = []
        with O.gates(None, record=log):
            O.factor_iteration_grads(*args64())
        _assert_gate_pattern(gates, log, "factor B=%d step %d" % (B, step))
        with O.gates(gates):
            _, _, g64, gd64, _ = O.factor_iteration_grads(*args64())
        for k, p in model.named_parameters():
            check(p.grad, g64[k], rtol=G_RTOL, atol_rel=G_ATOL, what="factor step %d grad vs gate-matched fp64 %s" % (step, k))
        for k, p in loss_f.discriminator.named_parameters():
            check(p.grad, gd64[k], rtol=G_RTOL, atol_rel=G_ATOL, what="factor step %d disc grad vs gate-matched fp64 %s" % (step, k))
        if step == 0:
            assert list(storer.keys()) == list(ref_logs.keys()), (list(storer.keys()), list(ref_logs.keys()))
            for k in ref_logs:
                np.testing.assert_allclose(storer[k][0], ref_logs[k].item(), rtol=5e-5, atol=1e-6, err_msg=k)
        for plist, mod, o_, lr_ in ((cpu, model, oc, lr), (dcpu, loss_f.discriminator, ocd, HP["lr_disc"])):
            for pc, (k, p) in zip(plist, mod.named_parameters()):
                pc.grad = p.grad.detach().cpu().clone()
            o_.step()
            for pc, (k, p) in zip(plist, mod.named_parameters()):
                d = (p.detach().cpu() - pc.detach()).abs()
                tol = 2 * pc.detach().abs() * 2.0 ** -23 + 4e-6 * lr_
                assert bool((d <= tol).all()), "param %s after step %d: GPU Adam vs torch CPU Adam: max diff %.3e" % (k, step, d.max().item())


GOLDEN = [("vae_mnist", "VAE", (1, 32, 32), 8, 2), ("betaB_mnist", "betaB", (1, 32, 32), 8, 2),
          ("btcvae_dsprites", "btcvae", (1, 64, 64), 8, 3), ("btcvae_celeba", "btcvae", (3, 64, 64), 6, 2),
          ("betaH_celeba", "betaH", (3, 64, 64), 4, 2), ("betaH_mnist_gaussian", "betaH", (1, 32, 32), 4, 1),
          ("betaH_mnist_laplace", "betaH", (1, 32, 32), 4, 1)]


@pytest.mark.parametrize("name,loss,img,B,steps", GOLDEN)
def test_trainer_vs_reference_golden(name, loss, img, B, steps):
    """Same seed -> same initial weights; same data and injected eps -> the reference's own
    recorded losses, storer scalars, gradient and parameter digests."""
    g = load(name)
    rec_dist = name.split("_")[-1] if name.endswith(("gaussian", "laplace")) else "bernoulli"
    model, opt, loss_f = _native(loss, img, int(g["seed"]), int(g["n_data"]), float(g["lr"]), rec_dist)
    for k, v in model.state_dict().items():   # same seed -> identical weights (sums: thread-count dependent order)
        d = tensor_digest(v)
        np.testing.assert_array_equal(d[2:], g["init_digest/" + k][2:], err_msg=k)
        np.testing.assert_allclose(d[:2], g["init_digest/" + k][:2], rtol=1e-12, err_msg=k)
    gen = torch.Generator().manual_seed(int(g["seed"]) + 1)
    for s in range(steps):
        data = torch.rand((B,) + tuple(img), generator=gen)
        storer = defaultdict(list)
        out = loss_f.fused_step(dev(data), model, opt, storer, eps=dev(torch.from_numpy(g["step%d/randn0" % s])))
        np.testing.assert_allclose(out.item(), g["step%d/loss" % s], rtol=2e-5 if s == 0 else 1e-3)
        for k, v in storer.items():
            np.testing.assert_allclose(v[0], g["step%d/storer/%s" % (s, k)], rtol=5e-5, atol=1e-6, err_msg=k)
        assert len(storer) == len([k for k in g if k.startswith("step%d/storer/" % s)])
        gr, ga = (2e-3, 2e-3) if s == 0 else (3e-2, 3e-2)
        for k, p in model.named_parameters():
            assert_digest_close(tensor_digest(p.grad), g["step%d/grad_digest/%s" % (s, k)], rtol=gr, atol_scale=ga,
                                what="%s step%d grad %s" % (name, s, k))
            assert_digest_close(tensor_digest(p), g["step%d/param_digest/%s" % (s, k)], rtol=1e-2, atol_scale=2e-2,
                                what="%s step%d param %s" % (name, s, k))
    model.eval()
    if name == "btcvae_dsprites":
        with torch.no_grad():
            recon, (mu, logvar), z = model(dev(data))
        np.testing.assert_allclose(mu.cpu().numpy(), g["eval/mu"], rtol=2e-3, atol=2e-4)
        assert torch.equal(z, mu)


@pytest.mark.parametrize("name,img", [("factor_dsprites", (1, 64, 64)), ("factor_celeba", (3, 64, 64))])
def test_factor_vs_reference_golden(name, img):
    g = load(name)
    model, opt, loss_f = _native("factor", img, int(g["seed"]), int(g["n_data"]), float(g["lr"]))
    for k, v in loss_f.discriminator.state_dict().items():
        d = tensor_digest(v)
        np.testing.assert_array_equal(d[2:], g["dinit_digest/" + k][2:], err_msg=k)
        np.testing.assert_allclose(d[:2], g["dinit_digest/" + k][:2], rtol=1e-12, err_msg=k)
    gen = torch.Generator().manual_seed(int(g["seed"]) + 1)
    for s in range(2):
        data = torch.rand((8,) + tuple(img), generator=gen)
        noise = (dev(torch.from_numpy(g["step%d/randn1" % s])), dev(torch.from_numpy(g["step%d/randn2" % s])),
                 torch.from_numpy(g["step%d/perms" % s]))
        storer = defaultdict(list)
        out = loss_f.call_optimize(dev(data), model, opt, storer, noise=noise)
        np.testing.assert_allclose(out.item(), g["step%d/loss" % s], rtol=2e-5 if s == 0 else 1e-3)
        for k, v in storer.items():
            np.testing.assert_allclose(v[0], g["step%d/storer/%s" % (s, k)], rtol=5e-5, atol=1e-6, err_msg=k)
        gr, ga = (2e-3, 2e-3) if s == 0 else (3e-2, 3e-2)
        for k, p in model.named_parameters():
            assert_digest_close(tensor_digest(p.grad), g["step%d/grad_digest/%s" % (s, k)], rtol=gr, atol_scale=ga,
                                what="%s step%d grad %s" % (name, s, k))
        for k, p in loss_f.discriminator.named_parameters():
            assert_digest_close(tensor_digest(p.grad), g["step%d/dgrad_digest/%s" % (s, k)], rtol=gr, atol_scale=ga,
                                what="%s step%d dgrad %s" % (name, s, k))
            assert_digest_close(tensor_digest(p), g["step%d/dparam_digest/%s" % (s, k)], rtol=1e-2, atol_scale=2e-2,
                                what="%s step%d dparam %s" % (name, s, k))


def test_reference_style_loop_matches_fused():
    """The reference's own control flow (model(x) -> loss_f(...) -> zero_grad -> backward ->
    step, training.py:152-158) works on the native model through the autograd wrappers and
    gives the same gradients as the fused path."""
    img, B = (3, 64, 64), 6
    m1, o1, l1 = _native("btcvae", img, 7, 202599, 5e-4)
    m2, o2, l2 = _native("btcvae", img, 7, 202599, 5e-4)
    gen = torch.Generator().manual_seed(3)
    data, eps = dev(torch.rand((B,) + img, generator=gen)), dev(torch.randn(B, 10, generator=gen))
    st1, st2 = defaultdict(list), defaultdict(list)
    recon, latent_dist, z = m1(data, eps=eps)
    loss = l1(data, recon, latent_dist, m1.training, st1, latent_sample=z)
    o1.zero_grad()
    loss.backward()
    g1 = {k: p.grad.clone() for k, p in m1.named_parameters()}
    o1.step()
    out = l2.fused_step(data, m2, o2, st2, eps=eps)
    np.testing.assert_allclose(loss.item(), out.item(), rtol=1e-5)
    assert list(st1.keys()) == list(st2.keys())
    for k in st1:
        np.testing.assert_allclose(st1[k][0], st2[k][0], rtol=2e-5, atol=1e-6, err_msg=k)
    for k, p in m2.named_parameters():
        # same conv kernels both ways; the FC core runs layer by layer here and as ONE launch in the fused step (fp32
        # summation order differs)
        check(g1[k], p.grad, rtol=1e-5, atol_rel=4e-6, what="autograd-vs-fused " + k)
    # encoder / decoder sub-module call surface (visualize.py:122-123,163,219)
    m1.eval()
    with torch.no_grad():
        mu, logvar = m1.encoder(data)
        rec = m1.decoder(mu)
        rec2, (mu2, lv2), z2 = m1(data)
    assert torch.equal(mu, mu2) and torch.equal(rec, rec2) and torch.equal(z2, mu2)


def test_trainer_api_epoch(tmp_path):
    """Trainer(model, optimizer, loss_f, device=...)(loader, epochs, checkpoint_every) end to
    end on a synthetic loader (training.py:64-135): losses log CSV + checkpoints."""
    import logging
    img, B = (1, 64, 64), 16
    model, opt, loss_f = _native("btcvae", img, 11, 737280, 5e-4)
    # the last batch of an epoch is smaller (no drop_last in the reference's loaders, datasets.py:67-71): the
    # engine switches batch size mid-epoch (new buffers, launch plans re-recorded)
    data = [(torch.rand((B,) + img), torch.zeros(B)) for _ in range(2)] + [(torch.rand((7,) + img), torch.zeros(7))]
    tr = Trainer(model, opt, loss_f, device=torch.device(DEV), logger=logging.getLogger("t"), save_dir=str(tmp_path),
                 is_progress_bar=False)
    tr(data, epochs=2, checkpoint_every=1)
    assert loss_f.n_train_steps == 6 and not model.training
    assert all(torch.isfinite(p).all() for p in model.parameters())
    log = (tmp_path / "train_losses.log").read_text().splitlines()
    assert log[0] == "Epoch,Loss,Value" and any(l.startswith("0,recon_loss,") for l in log)
    sd = torch.load(tmp_path / "model-1.pt")
    assert list(sd.keys())[0] == "encoder.conv1.weight" and sd["decoder.convT3.weight"].shape == (32, 1, 4, 4)
    # per-iteration API returns a python float
    model.train()
    v = tr._train_iteration(data[0][0], defaultdict(list))
    assert isinstance(v, float) and np.isfinite(v)


def test_no_silent_fallback():
    """The product fails loudly off-GPU: a CPU-resident native model refuses to compute."""
    model = init_specific_model("Burgess", (1, 32, 32), 10)
    with pytest.raises(_lib.DvaeHipError):
        model(torch.rand(2, 1, 32, 32))


@pytest.mark.parametrize("loss", ["btcvae", "betaB", "factor"])
def test_evaluator_losses_vs_oracle(loss, tmp_path):
    """Evaluator.compute_losses (evaluate.py:97-117): eval-mode forward (z = mean), is_train=False
    (annealing 1, storer always kept), every batch evaluated; vs the oracle."""
    import logging
    from disvae_amd.evaluate import Evaluator
    img, B = (1, 64, 64), 12
    model, opt, loss_f = _native(loss, img, 21, 737280, 5e-4)
    gen = torch.Generator().manual_seed(2)
    batches = [(torch.rand((B,) + img, generator=gen), torch.zeros(B)) for _ in range(2)]
    ev = Evaluator(model, loss_f, device=torch.device(DEV), logger=logging.getLogger("e"), save_dir=str(tmp_path),
                   is_progress_bar=False)
    model.train()
    _, losses = ev(batches, is_metrics=False, is_losses=True)
    assert model.training and loss_f.n_train_steps == 0
    torch.manual_seed(21)
    params = O.init_vae_params(img, 10)
    hp = dict(HP, n_data=737280)
    want = defaultdict(list)
    for data, _ in batches:
        x = data[:B // 2] if loss == "factor" else data
        with torch.no_grad():
            recon, (mu, logvar), z = O.vae_forward(params, x, None)
            if loss == "factor":
                dparams = O.clone_params({k: v.cpu() for k, v in loss_f.discriminator.state_dict().items()})
                rec = O.reconstruction_loss(x, recon); kl, _ = O.kl_normal_loss(mu, logvar)
                d_z = O.discriminator_forward(dparams, z)
                tc = (d_z[:, 0] - d_z[:, 1]).mean()
                want["recon_loss"].append(rec.item()); want["kl_loss"].append(kl.item())
                want["tc_loss"].append(tc.item()); want["loss"].append((rec + kl + 6.4 * tc).item())
            else:
                st = O.LossState(steps_anneal=HP["reg_anneal"])
                _, logs, _ = O.single_optimizer_loss(loss, hp, st, x, recon, mu, logvar, z, False)
                for k, v in logs.items():
                    want[k].append(v.item())
    for k, v in want.items():
        np.testing.assert_allclose(losses[k], sum(v) / len(v), rtol=5e-5, atol=1e-5, err_msg=k)
    assert (tmp_path / "test_losses.log").exists()


@pytest.mark.parametrize("mode", ["plan", "graph"])
@pytest.mark.parametrize("loss", ["btcvae", "betaB", "factor"])
def test_replay_matches_eager(loss, mode):
    """Replaying the captured iteration (disvae_amd/graph.py) runs the same kernels on the same
    inputs as the eager stream of launches: losses and parameters after 6 steps with injected noise
    (fresh batch, noise, permutations and annealing coefficient every step) are bit-identical."""
    img, B, D = (3, 64, 64), 16, 10
    runs = []
    for graph in (False, True):
        model, opt, loss_f = _native(loss, img, 33, 202599, 5e-4)
        loss_f.replay = mode if graph else None
        gen = torch.Generator().manual_seed(8)
        losses = []
        data = torch.empty((B,) + img, device=DEV)       # the batch keeps its address: plans are keyed on it
        for step in range(6):
            data.copy_(torch.rand((B,) + img, generator=gen))
            if loss == "factor":
                Bh = B // 2
                noise = (torch.randn(Bh, D, generator=gen).to(DEV), torch.randn(Bh, D, generator=gen).to(DEV),
                         torch.stack([torch.randperm(Bh, generator=gen) for _ in range(D)]))
                l = loss_f.call_optimize(data, model, opt, None, noise=noise)
            else:
                l = loss_f.fused_step(data, model, opt, None, eps=torch.randn(B, D, generator=gen).to(DEV))
            losses.append(l.item())
        if graph:
            assert loss_f._graphs.replays >= 2, "the iteration was never replayed"
        runs.append((losses, model.arena.flat.clone()))
    assert runs[0][0] == runs[1][0], (runs[0][0], runs[1][0])
    assert torch.equal(runs[0][1], runs[1][1])


@pytest.mark.parametrize("loss,img,B", [("btcvae", (3, 64, 64), 16), ("factor", (1, 64, 64), 24), ("VAE", (1, 32, 32), 9),
                                        ("betaB", (3, 64, 64), 300), ("betaH", (1, 64, 64), 1100)])
def test_conv_ends_inside_the_chain_launches_change_nothing(loss, img, B):
    """StepPolicy.fuse_ends (the 8x8 <-> 4x4 layers and their input gradients as prologue / epilogue of dvae_fc_chain_fwd / _bwd,
    up to its fuse_ends_max_rows rows per step; encoders.py:76-81, decoders.py:73-76) against the same steps with those four
    layers as launches of their own: same arithmetic, so losses and parameters after 4 steps are bit-identical.  The row limits
    are honoured: up to 256 rows both directions carry the conv ends (4 launches fewer per step), up to 1024 rows the forward
    chain only (2 fewer), above that none."""
    D = 10
    runs = []
    for fuse in (False, True):
        model, opt, loss_f = _native(loss, img, 21, 202599, 5e-4)
        assert model.engine.policy.fuse_ends, "the shipped configuration fuses the conv ends"
        loss_f.policy_override = {"fuse_ends": fuse}
        loss_f.replay = None                               # eager: every launch of every step goes through engine.call (counted)
        gen = torch.Generator().manual_seed(4)
        losses = []
        data = torch.empty((B,) + img, device=DEV)
        seen = []
        orig = _lib.call

        def spy(name, *a):
            seen.append(name)
            return orig(name, *a)
        import disvae_amd.engine as E
        E.call = spy
        try:
            for step in range(4):
                data.copy_(torch.rand((B,) + img, generator=gen))
                if loss == "factor":
                    Bh = B // 2
                    noise = (torch.randn(Bh, D, generator=gen).to(DEV), torch.randn(Bh, D, generator=gen).to(DEV),
                             torch.stack([torch.randperm(Bh, generator=gen) for _ in range(D)]))
                    l = loss_f.call_optimize(data, model, opt, None, noise=noise)
                else:
                    l = loss_f.fused_step(data, model, opt, None, eps=torch.randn(B, D, generator=gen).to(DEV))
                losses.append(l.item())
        finally:
            E.call = orig
        # launches of the 4x4 end per step: conv32_down at Hs = 4 (argument 7 of dvae_conv32_down) is gone exactly when fused
        n_chain = seen.count("dvae_fc_chain_fwd")
        assert n_chain >= 4
        runs.append((losses, model.arena.flat.clone(), model.arena.grad.clone(), len(seen)))
    assert runs[0][0] == runs[1][0], (runs[0][0], runs[1][0])
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])
    # (factor: the forward chain runs over both halves = B rows, the backward chain over B / 2)
    fwd = 2 if B <= 1024 else 0
    bwd = 2 if (B // 2 if loss == "factor" else B) <= 256 else 0
    assert runs[0][3] - runs[1][3] == 4 * (fwd + bwd), (runs[0][3], runs[1][3])


@pytest.mark.parametrize("mode", ["plan", "graph"])
@pytest.mark.parametrize("loss", ["btcvae", "factor"])
def test_replay_device_rng_trains(loss, mode, tmp_path):
    """Graph mode with the default on-device N(0,1) draws (captured torch.randn: fresh numbers on
    every replay) through the Trainer API: the loss falls and successive steps differ."""
    import logging
    img, B = (1, 64, 64), 32
    model, opt, loss_f = _native(loss, img, 5, 737280, 1e-3)
    tr = Trainer(model, opt, loss_f, device=torch.device(DEV), logger=logging.getLogger("g"), save_dir=str(tmp_path),
                 is_progress_bar=False, replay=mode)
    gen = torch.Generator().manual_seed(4)
    data = (torch.rand((B,) + img, generator=gen) > 0.7).float().to(DEV)
    losses = [tr._train_iteration(data, defaultdict(list)) for _ in range(40)]
    assert loss_f._graphs.replays >= 30
    assert all(np.isfinite(losses))
    assert len(set(losses[5:])) > 30                   # noise differs from replay to replay
    assert np.mean(losses[-5:]) < 0.95 * np.mean(losses[:5])


@pytest.mark.parametrize("loss,D", [("btcvae", 4), ("btcvae", 12), ("btcvae", 16), ("betaH", 16), ("factor", 7)])
def test_fused_step_other_latent_dims(loss, D):
    """--latent-dim other than 10 (main.py: any value; vae.py:30): the estimator / reparameterisation kernels take
    the latent dimension at run time (1..16)."""
    img, B, seed, n_data, lr = (1, 64, 64), 24, 99, 737280, 5e-4
    torch.manual_seed(seed)
    model = init_specific_model("Burgess", img, D)
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    hp = dict(HP, latent_dim=D, n_data=n_data)
    loss_f = get_loss_f(loss, device=torch.device(DEV), **hp)
    model.to(DEV).train()
    torch.manual_seed(seed)
    p0 = O.init_vae_params(img, D)
    gen = torch.Generator().manual_seed(seed + 1)
    data = torch.rand((B,) + img, generator=gen)
    st = O.LossState(steps_anneal=HP["reg_anneal"])
    c64 = lambda p: O.clone_params(p, dtype=torch.float64, requires_grad=True)
    storer = defaultdict(list)
    if loss == "factor":
        d0 = O.init_disc_params(D)
        Bh = B // 2
        eps1, eps2 = torch.randn(Bh, D, generator=gen), torch.randn(Bh, D, generator=gen)
        perms = torch.stack([torch.randperm(Bh, generator=gen) for _ in range(D)])
        ref_loss, ref_logs, g64, gd64, _ = O.factor_iteration_grads(hp, st, c64(p0), c64(d0), data.double(), eps1.double(),
                                                                    eps2.double(), list(perms))
        out = loss_f.call_optimize(dev(data), model, opt, storer, noise=(dev(eps1), dev(eps2), perms))
        for k, p in loss_f.discriminator.named_parameters():
            check(p.grad, gd64[k], rtol=1e-3, atol_rel=1e-4, what="D=%d disc grad %s" % (D, k))
    else:
        eps = torch.randn(B, D, generator=gen)
        ref_loss, ref_logs, g64, _ = O.train_iteration_grads(loss, hp, st, c64(p0), data.double(), eps.double())
        out = loss_f.fused_step(dev(data), model, opt, storer, eps=dev(eps))
    np.testing.assert_allclose(out.item(), ref_loss.item(), rtol=2e-5)
    assert list(storer.keys()) == list(ref_logs.keys())
    for k in ref_logs:
        np.testing.assert_allclose(storer[k][0], ref_logs[k].item(), rtol=5e-5, atol=1e-6, err_msg=k)
    for k, p in model.named_parameters():
        check(p.grad, g64[k], rtol=1e-3, atol_rel=1e-4, what="D=%d grad %s" % (D, k))


def test_autograd_path_after_fused_step_does_not_double_gradients():
    """after a fused step Parameter.grad aliases the gradient arena; a following reference-style iteration
    (model(x) -> loss -> zero_grad(set_to_none=False) -> backward) must still produce the plain gradient."""
    img, B = (1, 64, 64), 6
    m, o, l = _native("btcvae", img, 7, 737280, 5e-4)
    gen = torch.Generator().manual_seed(3)
    data, eps = dev(torch.rand((B,) + img, generator=gen)), dev(torch.randn(B, 10, generator=gen))
    l.fused_step(data, m, o, None, eps=eps)                       # .grad now aliases the arena
    m2, o2, l2 = _native("btcvae", img, 7, 737280, 5e-4)
    m2.load_state_dict(m.state_dict())
    l2.n_train_steps = l.n_train_steps
    data2, eps2 = dev(torch.rand((B,) + img, generator=gen)), dev(torch.randn(B, 10, generator=gen))
    recon, latent_dist, z = m(data2, eps=eps2)
    loss = l(data2, recon, latent_dist, True, None, latent_sample=z)
    o.zero_grad(set_to_none=False)
    loss.backward()
    l2.fused_step(data2, m2, o2, None, eps=eps2)                  # same iteration through the fused path
    for (k, p), (_, p2) in zip(m.named_parameters(), m2.named_parameters()):
        check(p.grad, p2.grad, rtol=1e-5, atol_rel=4e-6, what="grad after mixing paths " + k)
