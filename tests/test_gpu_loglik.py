"""GPU: per-image scores -- dvae_recon_rows against a float64 per-row oracle.reconstruction_loss, log_likelihood with explicit draws
against a gate-matched float64 restatement (oracle encoder / decoder / reconstruction_loss), per_image_losses against
Evaluator.compute_losses, seeded determinism without touching the global random states, and compute_log_likelihood between
training epochs beside an undisturbed training run."""
import ctypes
import logging
import math

import numpy as np
import pytest
import torch

from disvae_amd import _lib, Evaluator, log_likelihood, per_image_losses
from disvae_amd.data import DeviceImageLoader
from disvae_amd.engine import _stream
from disvae_amd.models.losses import get_loss_f
from disvae_amd.models.vae import init_specific_model
from disvae_amd.training import Trainer
from oracle import disvae_oracle as O
from oracle.gate_match import engine_gates, gate_mismatches

pytestmark = pytest.mark.gpu
DEV = "cuda"
HP = dict(rec_dist="bernoulli", reg_anneal=10000, betaH_B=4, betaB_initC=0, betaB_finC=25,
          betaB_G=1000, factor_G=6.4, latent_dim=10, lr_disc=1e-4, btcvae_A=1, btcvae_B=6.4, btcvae_G=1)


def seeded_model(img, D=10, seed=3):
    torch.manual_seed(seed)
    return init_specific_model("Burgess", img, D).to(DEV).eval()


def images(n, img, u8, seed):
    gen = torch.Generator().manual_seed(seed)
    if u8:
        return torch.randint(0, 256, (n,) + img, generator=gen, dtype=torch.uint8)
    return torch.rand((n,) + img, generator=gen)


def as_f64(x):
    return x.double() / 255 if x.dtype == torch.uint8 else x.double()


def recon_rows(recon, target, K, dist):
    n, row = target.shape[0], target[0].numel()
    out = torch.empty(n * K, dtype=torch.float32, device=DEV)
    need = ctypes.c_long()
    _lib.call("dvae_recon_rows_ws_floats", n, K, row, ctypes.addressof(need))
    ws = torch.full((need.value,), float("nan"), device=DEV) if need.value else None
    _lib.call("dvae_recon_rows", recon.data_ptr(), target.data_ptr(), int(target.dtype == torch.uint8), n, K, row, _lib.REC[dist],
              None if ws is None else ws.data_ptr(), out.data_ptr(), _stream())
    return out


# ---- 1. dvae_recon_rows -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3, 17])
@pytest.mark.parametrize("img", [(1, 32, 32), (3, 64, 64)])
@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("dist", ["bernoulli", "gaussian", "laplace"])
def test_recon_rows_vs_fp64_oracle(dist, u8, img, K):
    n_img = 5
    target = images(n_img, img, u8, seed=K).to(DEV)
    gen = torch.Generator().manual_seed(100 + K)
    recon = torch.rand((n_img * K,) + img, generator=gen)
    recon[0, 0, :2, :2] = torch.tensor([[0.0, 1.0], [1e-30, 1.0 - 2 ** -24]])   # the -100 clamp and the edges of (0, 1)
    recon = recon.to(DEV)
    got = recon_rows(recon, target, K, dist)
    again = recon_rows(recon, target, K, dist)
    assert torch.equal(got, again)                                       # fixed reduction order
    t64, r64 = as_f64(target.cpu()), recon.cpu().double()
    for i in range(n_img):
        for k in range(K):
            r = i * K + k
            want = O.reconstruction_loss(t64[i:i + 1], r64[r:r + 1], dist).item()
            assert abs(got[r].item() - want) <= 2e-6 * (abs(want) + 1.0), (i, k, got[r].item(), want)
    # a row's bits do not depend on the batch around it (rows per workgroup, grid)
    sub = recon_rows(recon[K:2 * K].contiguous(), target[1:2].contiguous(), K, dist)
    assert torch.equal(sub, got[K:2 * K])


@pytest.mark.parametrize("row_elems", [1000, 1300, 12288])
@pytest.mark.parametrize("K", [1, 8, 17])
def test_recon_rows_slices_and_row_groups_same_bits(row_elems, K):
    """Rows of one column slice, of several with a ragged last one, of twelve; K below, at and above the 8 rows of a workgroup
    (17: two full groups and a one-row tail).  Every row as the float64 sum, and bit for bit what one-image calls give."""
    n_img = 9
    target = images(n_img, (row_elems,), True, seed=K).to(DEV)
    recon = torch.rand((n_img * K, row_elems), generator=torch.Generator().manual_seed(row_elems + K)).to(DEV)
    got = recon_rows(recon, target, K, "bernoulli")
    assert torch.isfinite(got).all()
    for i in range(n_img):
        one = recon_rows(recon[i * K:(i + 1) * K].contiguous(), target[i:i + 1].contiguous(), K, "bernoulli")
        assert torch.equal(one, got[i * K:(i + 1) * K]), i
    t64, r64 = as_f64(target.cpu()), recon.cpu().double()
    for r in range(n_img * K):
        want = O.reconstruction_loss(t64[r // K:r // K + 1], r64[r:r + 1]).item()
        assert abs(got[r].item() - want) <= 2e-6 * abs(want), r


# ---- 2. log_likelihood against a gate-matched float64 restatement ----------------------------------------------------------
def _gates(model, B, prefix):
    return {k: v for k, v in engine_gates(model, B).items() if k.startswith(prefix)}


def _check_pattern(gates, log, what):
    n_diff, worst, ok = gate_mismatches(gates, log)
    assert ok, "%s: a ReLU gated differently than in fp64 at |pre-activation| = %.2e of the layer scale" % (what, worst)


def restated_loglik(model, x, eps, K, dist):
    """float64: encoder -> z = mu + exp(logvar / 2) eps -> decoder -> per-row reconstruction_loss -> log w -> logsumexp - log K,
    every ReLU gated as the engine gated it (oracle/gate_match.py).  Returns (log p^ [N], per-image tolerance scale [N])."""
    N, D = x.shape[0], model.latent_dim
    p64 = {k: v.detach().cpu().double() for k, v in model.state_dict().items()}
    xd = x.to(DEV)
    x64 = as_f64(x)
    with torch.no_grad():
        mu32, lv32 = model.encoder(xd)                                   # the engine's encoder at N rows: its gates
        enc = _gates(model, N, "encoder.")
        log = []
        with O.gates(None, record=log):
            O.encoder_forward(p64, x64)
        _check_pattern(enc, log, "encoder")
        with O.gates(enc):
            mu64, lv64 = O.encoder_forward(p64, x64)
        e64 = eps.double().reshape(N * K, D)
        z64 = mu64.repeat_interleave(K, 0) + torch.exp(0.5 * lv64.repeat_interleave(K, 0)) * e64
        z32 = mu32.repeat_interleave(K, 0) + torch.exp(0.5 * lv32.repeat_interleave(K, 0)) * eps.reshape(N * K, D).to(DEV)
        model.decoder(z32)                                               # the engine's decoder at N*K rows: its gates
        dec = _gates(model, N * K, "decoder.")
        log = []
        with O.gates(None, record=log):
            O.decoder_forward(p64, z64)
        _check_pattern(dec, log, "decoder")
        with O.gates(dec):
            r64 = O.decoder_forward(p64, z64)
    rec = torch.stack([O.reconstruction_loss(x64[r // K:r // K + 1], r64[r:r + 1], dist) for r in range(N * K)]).view(N, K)
    log_pz = (-0.5 * (z64 ** 2).sum(1)).view(N, K)
    log_qz = (-0.5 * (e64 ** 2 + lv64.repeat_interleave(K, 0)).sum(1)).view(N, K)
    lw = -rec + log_pz - log_qz
    ll = torch.logsumexp(lw, dim=1) - math.log(K)
    scale = (rec.abs() + log_pz.abs() + log_qz.abs()).max(dim=1).values
    return ll, scale


@pytest.mark.parametrize("img,D,N,K,dist,u8", [((1, 32, 32), 10, 37, 64, "bernoulli", False),
                                               ((1, 32, 32), 20, 37, 64, "gaussian", True),     # wide latent path
                                               ((3, 64, 64), 10, 3, 300, "laplace", False),     # one image spans two passes
                                               ((3, 64, 64), 20, 5, 40, "bernoulli", True)])
def test_log_likelihood_vs_fp64_restatement(img, D, N, K, dist, u8):
    model = seeded_model(img, D, seed=7)
    x = images(N, img, u8, seed=N + K)
    eps = torch.randn(N, K, D, generator=torch.Generator().manual_seed(K))
    got = log_likelihood(model, x, n_samples=K, rec_dist=dist, eps=eps).cpu().double()
    want, scale = restated_loglik(model, x, eps, K, dist)
    # tolerance: 2e-6 of the largest log w term of the image (tighter than 2e-5 x (|rec| + sum over k of the |log w terms|);
    # measured on an MI355X: at most 1e-3 of this bound is used)
    err = (got - want).abs() / (2e-6 * scale)
    assert err.max().item() <= 1.0, "worst error %.3f x tolerance (image %d: %r vs %r)" % (
        err.max().item(), int(err.argmax()), got[int(err.argmax())].item(), want[int(err.argmax())].item())
    # the eps of the explicit draws as [N*K, D]: the same bits
    assert torch.equal(log_likelihood(model, x, n_samples=K, rec_dist=dist, eps=eps.reshape(N * K, D)).cpu().double(), got)


# ---- 3. per_image_losses against Evaluator.compute_losses ------------------------------------------------------------------
@pytest.mark.parametrize("img,D,u8,dist", [((1, 64, 64), 10, True, "bernoulli"), ((3, 64, 64), 10, False, "gaussian"),
                                           ((1, 32, 32), 20, False, "laplace"), ((3, 32, 32), 10, True, "bernoulli")])
def test_per_image_losses_mean_is_the_evaluator_loss(img, D, u8, dist, tmp_path):
    model = seeded_model(img, D, seed=9)
    B = 16
    batches = [(images(B, img, u8, seed=20 + j), torch.zeros(B)) for j in range(3)]
    loss_f = get_loss_f("VAE", device=torch.device(DEV), n_data=3 * B, **dict(HP, rec_dist=dist, latent_dim=D))
    ev = Evaluator(model, loss_f, device=torch.device(DEV), logger=logging.getLogger("ll"), save_dir=str(tmp_path),
                   is_progress_bar=False)
    model.eval()
    losses = ev.compute_losses(batches)
    per = [per_image_losses(model, x, rec_dist=dist) for x, _ in batches]
    rec = torch.cat([p["recon"] for p in per]).cpu().double()
    kl = torch.cat([p["kl"] for p in per]).cpu().double()
    assert rec.shape == (3 * B,) and kl.shape == (3 * B, D)
    np.testing.assert_allclose(rec.mean().item(), losses["recon_loss"], rtol=1e-5)
    # a batch that is a view at an offset that is not 16-byte aligned gives the same bits
    x0 = batches[0][0].to(DEV)
    flat = torch.empty(x0.numel() + 1, dtype=x0.dtype, device=DEV)
    shifted = flat[1:].view(x0.shape)
    shifted.copy_(x0)
    assert shifted.data_ptr() % 16
    moved = per_image_losses(model, shifted, rec_dist=dist)
    assert torch.equal(moved["recon"], per[0]["recon"]) and torch.equal(moved["kl"], per[0]["kl"])
    for d in range(D):
        np.testing.assert_allclose(kl[:, d].mean().item(), losses["kl_loss_" + str(d)], rtol=1e-5, err_msg=str(d))


# ---- 4. determinism, random states, modes ----------------------------------------------------------------------------------
def test_seeded_runs_identical_and_global_rng_untouched(tmp_path):
    img, D, N, K = (1, 64, 64), 10, 11, 48
    model = seeded_model(img, D, seed=12).train()
    x = images(N, img, True, seed=3)
    cpu0, dev0 = torch.get_rng_state(), torch.cuda.get_rng_state()
    a = log_likelihood(model, x, n_samples=K, generator=torch.Generator(device=DEV).manual_seed(5))
    b = log_likelihood(model, x, n_samples=K, generator=torch.Generator(device=DEV).manual_seed(5))
    c = log_likelihood(model, x, n_samples=K, generator=torch.Generator(device=DEV).manual_seed(6))
    d = log_likelihood(model, x, n_samples=K)                             # default: a private generator seeded with 0
    e = log_likelihood(model, x, n_samples=K)
    assert torch.equal(a, b) and torch.equal(d, e) and not torch.equal(a, c)
    assert torch.isfinite(a).all() and (a < 0).all()
    loader = [(x[:6], None), (x[6:], None)]
    ev = Evaluator(model, get_loss_f("VAE", device=torch.device(DEV), **HP), device=torch.device(DEV),
                   logger=logging.getLogger("ll"), save_dir=str(tmp_path), is_progress_bar=False)
    r1 = ev.compute_log_likelihood(loader, n_samples=K, seed=3)
    r2 = ev.compute_log_likelihood(loader, n_samples=K, seed=3)
    assert r1 == r2 and r1["n_samples"] == K and r1["rec_dist"] == "bernoulli" and math.isfinite(r1["log_likelihood"])
    assert model.training                                                  # mode restored
    assert torch.equal(torch.get_rng_state(), cpu0) and torch.equal(torch.cuda.get_rng_state(), dev0)
    # Evaluator.__call__: the file only on request
    ev(loader, is_losses=False)
    assert not (tmp_path / "log_likelihood.log").exists()
    metric, losses = ev(loader, is_losses=False, is_log_likelihood=True, n_samples=K)
    assert (metric, losses) == (None, None)
    import json
    assert json.load(open(tmp_path / "log_likelihood.log")) == ev.compute_log_likelihood(loader, n_samples=K)
    assert model.training


# ---- 5. between training epochs ---------------------------------------------------------------------------------------------
class _LoglikHook:
    """Trainer's per-epoch hook slot (gif_visualizer: called after every epoch, save_reset() at the end)."""

    def __init__(self, ev, loader):
        self.ev, self.loader, self.values = ev, loader, []

    def __call__(self):
        self.values.append(self.ev.compute_log_likelihood(self.loader, n_samples=24, seed=1)["log_likelihood"])

    def save_reset(self):
        pass


def _train(tmp_path, loss, hooked):
    N, img, B = 2 * 64 + 7, (1, 64, 64), 64
    imgs = (torch.rand(N, 64, 64, generator=torch.Generator().manual_seed(5)) > 0.8).to(torch.uint8).numpy()
    torch.manual_seed(11)
    torch.cuda.manual_seed(11)
    loader = DeviceImageLoader(imgs, batch_size=B, shuffle=True, device=DEV)
    model = init_specific_model("Burgess", img, 10).to(DEV)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    loss_f = get_loss_f(loss, device=torch.device(DEV), n_data=N, **HP)
    d = tmp_path / ("hooked" if hooked else "plain")
    d.mkdir()
    hook = None
    if hooked:
        ev = Evaluator(model, loss_f, device=torch.device(DEV), logger=logging.getLogger("ll"), save_dir=str(d),
                       is_progress_bar=False)
        held_out = torch.from_numpy(imgs[:20]).unsqueeze(1)
        hook = _LoglikHook(ev, [(held_out[:13], None), (held_out[13:], None)])
    tr = Trainer(model, opt, loss_f, device=torch.device(DEV), logger=logging.getLogger("ll"), save_dir=str(d),
                 gif_visualizer=hook, is_progress_bar=False)
    gen0 = _lib.ALLOC_GEN[0]
    tr(loader, epochs=3, checkpoint_every=10)
    torch.cuda.synchronize()
    return dict(model=model, opt=opt, allocs=_lib.ALLOC_GEN[0] - gen0, log=open(d / "train_losses.log").read(),
                training=model.training, values=None if hook is None else hook.values)


@pytest.mark.parametrize("loss", ["btcvae", "VAE"])
def test_log_likelihood_between_epochs_leaves_training_untouched(tmp_path, loss):
    plain = _train(tmp_path, loss, hooked=False)
    hooked = _train(tmp_path, loss, hooked=True)
    for (k, p), q in zip(plain["model"].named_parameters(), hooked["model"].parameters()):
        assert torch.equal(p, q), k
    sa, sb = plain["opt"].state_dict()["state"], hooked["opt"].state_dict()["state"]
    for k in sa:
        for name in sa[k]:
            assert torch.equal(torch.as_tensor(sa[k][name]), torch.as_tensor(sb[k][name])), (k, name)
    assert plain["log"] == hooked["log"]
    assert plain["allocs"] == hooked["allocs"]                   # no extra plan invalidation: the scores' allocations are private
    assert plain["training"] == hooked["training"]
    assert len(hooked["values"]) == 3 and all(math.isfinite(v) for v in hooked["values"])
