"""GPU: the native visualizer -- dvae_image_grid_u8 against a numpy restatement of F.interpolate(nearest) + make_grid +
make_grid_img, the Visualizer's pictures against restated latents + model.decoder + that grid, GifTraversalsTraining beside an
undisturbed training run, and gif_traversals against a host restatement."""
import logging
import os
from collections import defaultdict

import numpy as np
import pytest
import torch
from PIL import Image, ImageSequence
from scipy import stats

from disvae_amd import _lib, Visualizer, GifTraversalsTraining
from disvae_amd import viz_helpers as VH
from disvae_amd.data import DeviceImageLoader
from disvae_amd.models.losses import get_loss_f
from disvae_amd.models.vae import init_specific_model
from disvae_amd.training import Trainer, LossesLogger

pytestmark = pytest.mark.gpu
DEV = "cuda"
HP = dict(rec_dist="bernoulli", reg_anneal=10000, betaH_B=4, betaB_initC=0, betaB_finC=25,
          betaB_G=1000, factor_G=6.4, latent_dim=10, lr_disc=1e-4, btcvae_A=1, btcvae_B=6.4, btcvae_G=1)


# ---- restatements ---------------------------------------------------------------------------------------------------------
def np_grid(imgs, nrow, padding=2, pad_value=0., f=1):
    """F.interpolate(nearest, integer factor) + make_grid + make_grid_img on the host, fp32 as torch computes it."""
    x = np.asarray(imgs, np.float32)
    x = x.repeat(f, axis=2).repeat(f, axis=3)
    if x.shape[1] == 1:
        x = np.repeat(x, 3, axis=1)
    n, _, H, W = x.shape
    if n == 1:
        g = x[0]
    else:
        xm = min(nrow, n)
        ym = -(-n // xm)
        g = np.full((3, ym * (H + padding) + padding, xm * (W + padding) + padding), np.float32(pad_value), np.float32)
        for k in range(n):
            y, c = divmod(k, xm)
            g[:, y * (H + padding) + padding:y * (H + padding) + padding + H,
              c * (W + padding) + padding:c * (W + padding) + padding + W] = x[k]
    v = (g * np.float32(255)).astype(np.float32)
    v = (v + np.float32(0.5)).astype(np.float32)
    return np.clip(v, 0, 255).astype(np.uint8).transpose(1, 2, 0)


def traverse_line(latent_dim, idx, n_samples, max_traversal=0.475, post=None):
    """utils/visualize.py _get_traversal_range + _traverse_line; post = (sample [D], mean [D], std [D]) host tensors."""
    def rng(mean=0, std=1):
        m = max_traversal
        if m < 0.5:
            m = stats.norm.ppf((1 - 2 * m) / 2, loc=mean, scale=std)
        return (-1 * m, m)
    if post is None:
        samples = torch.zeros(n_samples, latent_dim)
        trav = torch.linspace(*rng(), steps=n_samples)
    else:
        samples = post[0].reshape(1, -1).repeat(n_samples, 1)
        trav = torch.linspace(*rng(mean=post[1][idx], std=post[2][idx]), steps=n_samples)
    for i in range(n_samples):
        samples[i, idx] = trav[i]
    return samples


def decode(model, z):
    with torch.no_grad():
        return model.decoder(z.to(DEV)).cpu().numpy()


def seeded_model(img, D=10, seed=3):
    torch.manual_seed(seed)
    return init_specific_model("Burgess", img, D).to(DEV).eval()


def write_losses(model_dir, D, seed=0):
    log = LossesLogger(os.path.join(model_dir, "train_losses.log"))
    rng = np.random.default_rng(seed)
    st = defaultdict(list)
    for i in range(D):
        st["kl_loss_" + str(i)].append(float(rng.uniform(0, 3)))
    log.log(0, st)
    return [st["kl_loss_" + str(i)][0] for i in range(D)]


def reorder(rows, losses):
    """sort_list_by_other(rows, losses): rows by decreasing loss."""
    return [rows[r] for _, r in sorted(zip(losses, range(len(rows))), reverse=True)]


def read_png(path):
    return np.asarray(Image.open(path).convert("RGB"))


# ---- 1. the grid kernel ---------------------------------------------------------------------------------------------------
def _inputs(n, C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, C, H, W, generator=g).numpy()
    # exact 0 / 1 and values whose x * 255 + 0.5 lands within an ulp or two of k + 0.5 and k + 1 (an FMA or another rounding
    # of the conversion moves these first)
    special = [0.0, 1.0]
    for k in range(256):
        for c in ((k + 0.5) / 255, k / 255):
            b = np.float32(c)
            special += [b, np.nextafter(b, np.float32(2)), np.nextafter(b, np.float32(-1))]
    special = np.clip(np.array(special, np.float32), 0, 1)
    flat = x.reshape(-1)
    pos = torch.randperm(flat.size, generator=g).numpy()[:special.size]
    flat[pos[:min(special.size, flat.size)]] = special[:min(special.size, flat.size)]
    return x


@pytest.mark.parametrize("C,H", [(1, 32), (3, 32), (1, 64), (3, 64)])
def test_grid_kernel_matches_make_grid(C, H):
    x = _inputs(100, C, H, H, seed=C * 100 + H)
    xd = torch.from_numpy(x).to(DEV)
    for n in (1, 7, 64, 100):
        for nrow in (1, 8, 10):
            for f in (1, 2):
                for pad in (0., 1.):
                    got = VH.image_grid_u8(xd[:n], nrow=nrow, pad_value=pad, upsample=f).cpu().numpy()
                    want = np_grid(x[:n], nrow, 2, pad, f)
                    assert got.dtype == np.uint8 and np.array_equal(got, want), (n, nrow, f, pad)
    # uint8 pixels (dvae_u8_to_f32 first), another padding, and an output that is not 16-byte aligned (byte stores)
    u8 = (torch.from_numpy(x[:7]) * 255).to(torch.uint8)
    got = VH.image_grid_u8(u8.to(DEV), nrow=3, padding=5, pad_value=0.5).cpu().numpy()
    assert np.array_equal(got, np_grid(u8.numpy().astype(np.float32) / np.float32(255), 3, 5, 0.5))
    h, w = VH.grid_shape(7, H, H, 3)
    raw = torch.full((h * w * 3 + 1,), 77, dtype=torch.uint8, device=DEV)
    _lib.call("dvae_image_grid_u8", xd.data_ptr(), 7, C, H, H, 3, 2, 1.0, 1, raw.data_ptr() + 1,
              torch.cuda.current_stream().cuda_stream)
    raw = raw.cpu().numpy()
    assert raw[0] == 77 and np.array_equal(raw[1:].reshape(h, w, 3), np_grid(x[:7], 3, 2, 1.0))


# ---- 2. the Visualizer's pictures -----------------------------------------------------------------------------------------
def _recording(vis):
    seen = []
    orig = vis.native.decode

    def rec(z):
        seen.append(z.detach().cpu().clone())
        return orig(z)
    vis.native.decode = rec
    return seen


def test_traversals_reconstruct_samples(tmp_path):
    img, D = (3, 64, 64), 10
    model = seeded_model(img, D)
    d = str(tmp_path)
    vis = Visualizer(model, "celeba", d, upsample_factor=2)
    seen = _recording(vis)
    pad = 1 - 1                                               # celeba: white background

    # prior traversals
    vis.traversals(n_per_latent=8)
    z = torch.cat([traverse_line(D, i, 8) for i in range(D)])
    assert torch.equal(seen[-1], z)
    assert np.array_equal(read_png(os.path.join(d, "prior_traversals.png")), np_grid(decode(model, z), 8, 2, pad, 2))

    # posterior traversals of one image
    data = torch.rand(16, *img, generator=torch.Generator().manual_seed(1))
    vis.traversals(data=data[:1], n_per_latent=6, n_latents=4)
    with torch.no_grad():
        mu, lv = model.encoder(data[:1].to(DEV))
        s = model.reparameterize(mu, lv)
        post = (s.cpu()[0], mu.cpu()[0], torch.exp(lv / 2).cpu()[0])
    z = torch.cat([traverse_line(D, i, 6, post=post) for i in range(D)])
    assert torch.equal(seen[-1], z)
    want = np_grid(decode(model, z)[:24], 6, 2, pad, 2)
    assert np.array_equal(read_png(os.path.join(d, "posterior_traversals.png")), want)

    # reconstructions
    vis.reconstruct(data, size=(4, 4))
    with torch.no_grad():
        recs = model(data[:8].to(DEV))[0].cpu().numpy()
    want = np_grid(np.concatenate([data[:8].numpy(), recs]), 4, 2, pad, 2)
    assert np.array_equal(read_png(os.path.join(d, "reconstruct.png")), want)
    assert np.array_equal(vis.reconstruct(data, size=(4, 4), is_force_return=True), want)

    # samples: drawn from the CPU generator
    torch.manual_seed(42)
    vis.generate_samples(size=(3, 5))
    torch.manual_seed(42)
    z = torch.randn(15, D)
    assert torch.equal(seen[-1], z)
    assert np.array_equal(read_png(os.path.join(d, "samples.png")), np_grid(decode(model, z), 5, 2, pad, 2))

    # uint8 pixel batches (DeviceImageLoader) for data_samples
    u8 = (data * 255).to(torch.uint8)
    vis.data_samples(u8.to(DEV), size=(2, 4))
    want = np_grid(u8[:8].numpy().astype(np.float32) / np.float32(255), 4, 2, pad, 2)
    assert np.array_equal(read_png(os.path.join(d, "data_samples.png")), want)


def test_reconstruct_traverse(tmp_path):
    img, D = (1, 64, 64), 10
    model = seeded_model(img, D, seed=4)
    d = str(tmp_path)
    losses = write_losses(d, D)
    vis = Visualizer(model, "dsprites", d, loss_of_interest="kl_loss_")
    assert vis.losses == losses
    data = (torch.rand(16, *img, generator=torch.Generator().manual_seed(2)) > 0.7).float()
    n_per, n_lat = 5, 6
    vis.reconstruct_traverse(data, n_per_latent=n_per, n_latents=n_lat)
    with torch.no_grad():
        recs = model(data[:n_per].to(DEV))[0].cpu().numpy()
        mu, lv = model.encoder(data[:1].to(DEV))
        post = (model.reparameterize(mu, lv).cpu()[0], mu.cpu()[0], torch.exp(lv / 2).cpu()[0])
    top = np_grid(np.concatenate([data[:n_per].numpy(), recs]), n_per, 2, 1)
    dec = decode(model, torch.cat([traverse_line(D, i, n_per, post=post) for i in range(D)]))
    rows = reorder(list(dec.reshape(D, n_per, *img)), losses)
    bottom = np_grid(np.concatenate(rows)[:n_per * n_lat], n_per, 2, 1)
    want = np.concatenate([top, bottom], axis=0)
    assert np.array_equal(read_png(os.path.join(d, "reconstruct_traverse.png")), want)
    vis.reconstruct_traverse(data, n_per_latent=n_per, n_latents=n_lat, is_show_text=True)
    got = read_png(os.path.join(d, "reconstruct_traverse.png"))
    assert got.shape == (want.shape[0], want.shape[1] + 100, 3) and np.array_equal(got[:, :want.shape[1]], want)
    assert (got[:, want.shape[1]:] != 255).any()                 # the labels were drawn


# ---- 3. GifTraversalsTraining beside a training run -----------------------------------------------------------------------
def _train(tmp_path, loss, gif):
    N, img, B = 2 * 64 + 7, (1, 64, 64), 64                    # B = 64, then a 7-image last batch every epoch
    imgs = (torch.rand(N, 64, 64, generator=torch.Generator().manual_seed(5)) > 0.8).to(torch.uint8).numpy()
    torch.manual_seed(11)
    torch.cuda.manual_seed(11)
    loader = DeviceImageLoader(imgs, batch_size=B, shuffle=True, device=DEV)
    model = init_specific_model("Burgess", img, 10).to(DEV)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    loss_f = get_loss_f(loss, device=torch.device(DEV), n_data=N, **HP)
    d = tmp_path / ("gif" if gif else "plain")
    d.mkdir()
    viz, captured = None, []
    if gif:
        viz = GifTraversalsTraining(model, "dsprites", str(d))
        save_reset = viz.save_reset

        def capture():
            captured.extend(viz.frames())
            save_reset()
        viz.save_reset = capture
    tr = Trainer(model, opt, loss_f, device=torch.device(DEV), logger=logging.getLogger("viz"), save_dir=str(d),
                 gif_visualizer=viz, is_progress_bar=False)
    gen0 = _lib.ALLOC_GEN[0]
    tr(loader, epochs=3, checkpoint_every=10)
    torch.cuda.synchronize()
    return dict(model=model, opt=opt, loss_f=loss_f, dir=d, frames=captured, allocs=_lib.ALLOC_GEN[0] - gen0,
                log=open(d / "train_losses.log").read(), training=model.training)


def _states_equal(a, b):
    sa, sb = a.state_dict()["state"], b.state_dict()["state"]
    assert sa.keys() == sb.keys()
    for k in sa:
        for name in sa[k]:
            assert torch.equal(torch.as_tensor(sa[k][name]), torch.as_tensor(sb[k][name])), (k, name)


@pytest.mark.parametrize("loss", ["btcvae", "factor"])
def test_gif_hook_leaves_training_untouched(tmp_path, loss):
    plain = _train(tmp_path, loss, gif=False)
    hooked = _train(tmp_path, loss, gif=True)
    for (k, p), q in zip(plain["model"].named_parameters(), hooked["model"].parameters()):
        assert torch.equal(p, q), k
    _states_equal(plain["opt"], hooked["opt"])
    if loss == "factor":
        for p, q in zip(plain["loss_f"].discriminator.parameters(), hooked["loss_f"].discriminator.parameters()):
            assert torch.equal(p, q)
        _states_equal(plain["loss_f"].optimizer_d, hooked["loss_f"].optimizer_d)
    assert plain["log"] == hooked["log"]
    assert plain["allocs"] == hooked["allocs"]                   # no extra plan invalidation: the frames' allocations are private
    assert plain["training"] == hooked["training"]
    # the GIF: 3 frames of a 10 x 10 grid of 64 x 64 images, decoding back exactly (grey) to the in-memory grids
    frames = hooked["frames"]
    assert len(frames) == 3 and all(f.shape == (662, 662, 3) for f in frames)
    im = Image.open(hooked["dir"] / "training.gif")
    back = [np.asarray(f.convert("RGB")) for f in ImageSequence.Iterator(im)]
    assert len(back) == 3 and all(np.array_equal(x, y) for x, y in zip(back, frames))
    # the last frame is the prior traversal of the final parameters
    model = hooked["model"].eval()
    z = torch.cat([traverse_line(10, i, 10) for i in range(10)])
    assert np.array_equal(frames[-1], np_grid(decode(model, z), 10, 2, 1))


# ---- 4. gif_traversals ----------------------------------------------------------------------------------------------------
def test_gif_traversals_matches_host_restatement(tmp_path):
    img, D, n_img, n_per = (1, 64, 64), 10, 4, 5
    model = seeded_model(img, D, seed=6)
    d = str(tmp_path)
    losses = write_losses(d, D, seed=1)
    vis = Visualizer(model, "dsprites", d, loss_of_interest="kl_loss_")
    data = (torch.rand(n_img, *img, generator=torch.Generator().manual_seed(3)) > 0.7).float()
    frames = vis.gif_traversals(data, n_latents=7, n_per_gif=n_per)
    with torch.no_grad():
        mu, lv = model.encoder(data.to(DEV))
        s, std = model.reparameterize(mu, lv).cpu(), torch.exp(lv / 2).cpu()
    mu = mu.cpu()
    z = torch.cat([traverse_line(D, dim, n_per, post=(s[i], mu[i], std[i])) for i in range(n_img) for dim in range(D)])
    dec = decode(model, z).reshape(n_img, D, n_per, *img)
    cols = [[] for _ in range(n_per)]
    for i in range(n_img):
        grid = np_grid(np.concatenate(reorder(list(dec[i]), losses))[:7 * n_per], n_per, 2, 1)
        for j in range(n_per):
            x0 = (j + 1) * 2 + j * 64
            cols[j].append(grid[:, x0:x0 + 64])
    want = [VH.concatenate_pad(c, 2, 255, axis=1) for c in cols]
    assert len(frames) == n_per and all(np.array_equal(a, b) for a, b in zip(frames, want))
    back = [np.asarray(f.convert("RGB")) for f in ImageSequence.Iterator(Image.open(os.path.join(d, "posterior_traversals.gif")))]
    assert len(back) == n_per and all(np.array_equal(a, b) for a, b in zip(back, want))
