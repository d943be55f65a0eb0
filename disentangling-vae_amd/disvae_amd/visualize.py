"""Visualizer and per-epoch training GIF with the API of utils/visualize.py, on the native model.

Every picture is decoded by the HIP engine and gridded on the device (dvae_image_grid_u8: F.interpolate(nearest) + make_grid +
make_grid_img in one launch, bit for bit); one device-to-host copy of uint8 bytes per picture.  The reference pulls every decoded
batch to the host as fp32 and grids it on the CPU.

The passes run on a PRIVATE engine over the model's parameter arena (``_NativePasses``): the model's own engine keeps its
workspaces, and the launch plans the training step recorded at its batch sizes stay valid, so ``GifTraversalsTraining`` can be
handed to the unchanged ``Trainer`` without moving a bit of the training run.
"""
import contextlib
import os

import numpy as np
import torch
from PIL import Image

from . import _lib
from .engine import VAEEngine
from .viz_helpers import (FPS_GIF, add_labels, check_upsample, concatenate_pad, get_background, image_grid_u8,  # noqa: F401
                          read_loss_from_file, save_gif, save_png, sort_list_by_other, to_f32_device)

TRAIN_FILE = "train_losses.log"
DECIMAL_POINTS = 3
GIF_FILE = "training.gif"
PLOT_NAMES = dict(generate_samples="samples.png",
                  data_samples="data_samples.png",
                  reconstruct="reconstruct.png",
                  traversals="traversals.png",
                  reconstruct_traverse="reconstruct_traverse.png",
                  gif_traversals="posterior_traversals.gif",)


@contextlib.contextmanager
def _private_allocs():
    """Allocations of the private engine free nothing a recorded launch plan points into (plans are recorded by the training
    step on the model's own engine): they do not count as a reallocation (_lib.ALLOC_GEN), which would make the next training
    step record its plan again."""
    gen = _lib.ALLOC_GEN[0]
    try:
        yield
    finally:
        _lib.ALLOC_GEN[0] = gen


class _NativePasses:
    """Encoder / decoder passes of a native VAE for the pictures: a VAEEngine of its own over the model's parameters (always
    the current ones), with ONE workspace of up to MAX_ROWS rows, grown to the next power of two as requests need; larger
    requests run in chunks of MAX_ROWS rows."""

    MAX_ROWS = 256

    def __init__(self, model):
        self.model = model
        self._eng = None
        self._rows = 0

    def check_device(self):
        """The model's device; DvaeHipError unless it is a GPU (there is no CPU path)."""
        dev = self.model.arena.flat.device
        if dev.type != "cuda":
            raise _lib.DvaeHipError("the native VAE computes only on an MI355X (model is on %s); move it with .to('cuda') -- "
                                    "there is no CPU fallback" % dev)
        return dev

    def _buffers(self, rows):
        m = self.model
        self.check_device()
        if self._eng is None:
            self._eng = VAEEngine(m.img_size, m.latent_dim, m.arena)
        want = min(self.MAX_ROWS, 1 << max(0, int(rows) - 1).bit_length())
        if want > self._rows:
            self._eng._bufs.clear()
            self._rows = want
        return self._eng, self._eng.buffers(self._rows)

    def decode(self, z):
        """z [N, D] fp32 on the device -> sigmoid outputs [N, C, H, W].  A request of at most MAX_ROWS rows returns a view of
        the workspace (valid until the next pass)."""
        N = z.shape[0]
        with _private_allocs():
            eng, buf = self._buffers(N)
            if N <= self.MAX_ROWS:
                eng.decode(z.contiguous(), buf)
                return buf.recon[:N]
            out = torch.empty((N,) + self.model.img_size, dtype=torch.float32, device=z.device)
            for lo in range(0, N, self.MAX_ROWS):
                hi = min(N, lo + self.MAX_ROWS)
                eng.decode(z[lo:hi].contiguous(), buf)
                out[lo:hi].copy_(buf.recon[:hi - lo])
            return out

    def encode(self, x):
        """x [N, C, H, W] fp32 on the device -> (mu, logvar), each [N, D] (model.encoder)."""
        N = x.shape[0]
        D = self.model.latent_dim
        mu = torch.empty((N, D), dtype=torch.float32, device=x.device)
        logvar = torch.empty_like(mu)
        with _private_allocs():
            eng, buf = self._buffers(N)
            for lo in range(0, N, self.MAX_ROWS):
                hi = min(N, lo + self.MAX_ROWS)
                eng.encode(x[lo:hi].contiguous(), buf)
                eng.reparam(buf, None, n=hi - lo)
                mu[lo:hi].copy_(buf.mu[:hi - lo])
                logvar[lo:hi].copy_(buf.logvar[:hi - lo])
        return mu, logvar

    def forward(self, x):
        """model(x)[0]: the reconstructions, with the N(0, 1) draw of the training mode as VAE.forward makes it."""
        N = x.shape[0]
        eps = None
        if self.model.training:
            eps = torch.randn(N, self.model.latent_dim, dtype=torch.float32, device=x.device)
        out = torch.empty_like(x)
        with _private_allocs():
            eng, buf = self._buffers(N)
            for lo in range(0, N, self.MAX_ROWS):
                hi = min(N, lo + self.MAX_ROWS)
                eng.encode(x[lo:hi].contiguous(), buf)
                eng.reparam(buf, None if eps is None else eps[lo:hi], n=hi - lo)
                eng.decode(buf.z[:hi - lo], buf, staged=True)
                out[lo:hi].copy_(buf.recon[:hi - lo])
        return out


class Visualizer():
    def __init__(self, model, dataset, model_dir,
                 save_images=True,
                 loss_of_interest=None,
                 display_loss_per_dim=False,
                 max_traversal=0.475,  # corresponds to ~2 for standard normal
                 upsample_factor=1):
        """utils/visualize.py:21-77: pictures of a native VAE's samples, reconstructions and latent traversals, written to
        ``model_dir`` (``save_images``) or returned as uint8 [h, w, 3] arrays.  ``max_traversal`` < 0.5 is a quantile of the
        traversed distribution, >= 0.5 an absolute value; ``upsample_factor`` an integer nearest-neighbour factor;
        ``loss_of_interest`` (e.g. "kl_loss_") orders the latent dimensions by that loss of the last epoch in train_losses.log."""
        self.model = model
        self.latent_dim = self.model.latent_dim
        self.max_traversal = max_traversal
        self.save_images = save_images
        self.model_dir = model_dir
        self.dataset = dataset
        self.pad_value = 1 - get_background(dataset)
        self.upsample_factor = check_upsample(upsample_factor)
        self.display_loss_per_dim = display_loss_per_dim
        self.losses = None
        if loss_of_interest is not None:
            self.losses = read_loss_from_file(os.path.join(self.model_dir, TRAIN_FILE), loss_of_interest)
        self.native = _NativePasses(model)
        self._traversal_cache = {}

    @property
    def device(self):
        return self.model.arena.flat.device

    # ---- latents ----------------------------------------------------------------------------------------------------------
    def _get_traversal_range(self, mean=0, std=1):
        """Return the corresponding traversal range in absolute terms (a quantile of N(mean, std^2) when max_traversal < 0.5)."""
        max_traversal = self.max_traversal
        if max_traversal < 0.5:
            from scipy import stats
            max_traversal = (1 - 2 * max_traversal) / 2
            max_traversal = stats.norm.ppf(max_traversal, loc=mean, scale=std)
        return (-1 * max_traversal, max_traversal)

    def _traverse_line(self, idx, n_samples, post=None):
        """(n_samples, latent_dim) host fp32 latents traversing dimension idx; the other dimensions at 0 (prior, post None) or
        at the posterior sample of one image, post = (sample [D], mean [D], std [D]) host fp32 tensors."""
        if post is None:
            samples = torch.zeros(n_samples, self.latent_dim)
            traversals = torch.linspace(*[float(v) for v in self._get_traversal_range()], steps=n_samples)
        else:
            sample, mean, std = post
            samples = sample.reshape(1, -1).repeat(n_samples, 1)
            rng = self._get_traversal_range(mean=np.float32(mean[idx].item()), std=np.float32(std[idx].item()))
            traversals = torch.linspace(*[float(v) for v in rng], steps=n_samples)
        samples[:, idx] = traversals
        return samples

    def _posteriors(self, data):
        """Posterior (sample, mean, std) of every image of data, on the host: ONE encoder pass, one copy."""
        x = to_f32_device(data, self.device)
        mu, logvar = self.native.encode(x)
        samples = self.model.reparameterize(mu, logvar)
        std = torch.exp(logvar / 2)
        host = torch.stack([samples, mu, std]).cpu()
        return [(host[0, i], host[1, i], host[2, i]) for i in range(x.shape[0])]

    def _traversal_latents(self, n_per_latent, post=None):
        return torch.cat([self._traverse_line(dim, n_per_latent, post) for dim in range(self.latent_dim)], dim=0)

    # ---- pictures ---------------------------------------------------------------------------------------------------------
    def _reorder(self, decoded, n_per_latent):
        """Rows of traversals (n_per_latent images each) ordered by decreasing loss of interest (sort_list_by_other)."""
        if self.losses is None:
            raise ValueError("is_reorder_latents needs the losses to order by: pass loss_of_interest")
        n_rows = decoded.shape[0] // n_per_latent
        key = ("order", n_rows, decoded.device)
        idx = self._traversal_cache.get(key)
        if idx is None:                                   # (uploaded once from pinned memory: no host synchronisation)
            host = torch.tensor(sort_list_by_other(list(range(n_rows)), self.losses), dtype=torch.long).pin_memory()
            idx = self._traversal_cache[key] = (host, host.to(decoded.device, non_blocking=True))
        rows = decoded.reshape(n_rows, n_per_latent, *decoded.shape[1:]).index_select(0, idx[1])
        return rows.reshape(-1, *decoded.shape[1:])

    def _grid(self, to_plot, size):
        """uint8 [h, w, 3] device grid of to_plot on a size[0] x size[1] layout (the checks of _save_or_return)."""
        if size[0] * size[1] != to_plot.shape[0]:
            raise ValueError("Wrong size {} for datashape {}".format(size, tuple(to_plot.shape)))
        return image_grid_u8(to_plot, nrow=size[1], pad_value=self.pad_value, upsample=self.upsample_factor)

    def _save_or_return(self, to_plot, size, filename, is_force_return=False):
        """Create plot and save or return it."""
        img = self._grid(to_plot, size).cpu().numpy()
        if self.save_images and not is_force_return:
            save_png(img, os.path.join(self.model_dir, filename))
        else:
            return img

    def _decode_latents(self, latent_samples):
        """Host latents [N, D] -> device images [N, C, H, W] (one host-to-device copy, one decoder pass)."""
        return self.native.decode(latent_samples.to(self.device, torch.float32))

    def generate_samples(self, size=(8, 8)):
        """Plot generated samples from the prior (drawn from the CPU generator, as the reference does) and decoding."""
        prior_samples = torch.randn(size[0] * size[1], self.latent_dim)
        generated = self._decode_latents(prior_samples)
        return self._save_or_return(generated, size, PLOT_NAMES["generate_samples"])

    def data_samples(self, data, size=(8, 8)):
        """Plot samples from the dataset (data: [N, C, H, W] fp32 in [0, 1] or uint8 pixels)."""
        data = data[:size[0] * size[1], ...]
        return self._save_or_return(to_f32_device(data, self.device), size, PLOT_NAMES["data_samples"])

    def reconstruct(self, data, size=(8, 8), is_original=True, is_force_return=False):
        """Reconstructions of data through the model (upper half of the rows the originals when is_original)."""
        if is_original:
            if size[0] % 2 != 0:
                raise ValueError("Should be even number of rows when showing originals not {}".format(size[0]))
            n_samples = size[0] // 2 * size[1]
        else:
            n_samples = size[0] * size[1]
        originals = to_f32_device(data[:n_samples, ...], self.device)
        recs = self.native.forward(originals)
        to_plot = torch.cat([originals, recs]) if is_original else recs
        return self._save_or_return(to_plot, size, PLOT_NAMES["reconstruct"], is_force_return=is_force_return)

    def _traversal_grid(self, data, is_reorder_latents, n_per_latent, n_latents):
        """Device uint8 grid of traversals() (prior latents are built and uploaded once per n_per_latent)."""
        n_latents = n_latents if n_latents is not None else self.model.latent_dim
        if data is None:
            key = (n_per_latent, self.device)
            z = self._traversal_cache.get(key)
            if z is None:
                host = self._traversal_latents(n_per_latent).pin_memory()
                z = self._traversal_cache[key] = (host, host.to(self.device, non_blocking=True))
            decoded = self.native.decode(z[1])
        else:
            if data.size(0) > 1:
                raise ValueError("Every value should be sampled from the same posterior, but {} datapoints given."
                                 .format(data.size(0)))
            decoded = self._decode_latents(self._traversal_latents(n_per_latent, self._posteriors(data)[0]))
        if is_reorder_latents:
            decoded = self._reorder(decoded, n_per_latent)
        decoded = decoded[:n_per_latent * n_latents]
        return self._grid(decoded, (n_latents, n_per_latent))

    def traversals(self, data=None, is_reorder_latents=False, n_per_latent=8, n_latents=None, is_force_return=False):
        """Grid whose rows traverse the latent dimensions one by one: from the prior (data None) or from the posterior of the
        single image in data."""
        grid = self._traversal_grid(data, is_reorder_latents, n_per_latent, n_latents)
        sampling_type = "prior" if data is None else "posterior"
        filename = "{}_{}".format(sampling_type, PLOT_NAMES["traversals"])
        img = grid.cpu().numpy()
        if self.save_images and not is_force_return:
            save_png(img, os.path.join(self.model_dir, filename))
        else:
            return img

    def reconstruct_traverse(self, data, is_posterior=True, n_per_latent=8, n_latents=None, is_show_text=False):
        """One row of originals, one of reconstructions, then the traversals of the latent dimensions (ordered by the loss of
        interest), optionally labelled with that loss."""
        n_latents = n_latents if n_latents is not None else self.model.latent_dim
        reconstructions = self.reconstruct(data[:2 * n_per_latent, ...], size=(2, n_per_latent), is_force_return=True)
        traversals = self.traversals(data=data[0:1, ...] if is_posterior else None, is_reorder_latents=True,
                                     n_per_latent=n_per_latent, n_latents=n_latents, is_force_return=True)
        concatenated = Image.fromarray(np.concatenate((reconstructions, traversals), axis=0))
        if is_show_text:
            losses = sorted(self.losses, reverse=True)[:n_latents]
            labels = ['orig', 'recon'] + ["KL={:.4f}".format(l) for l in losses]
            concatenated = add_labels(concatenated, labels)
        concatenated.save(os.path.join(self.model_dir, PLOT_NAMES["reconstruct_traverse"]))

    def gif_traversals(self, data, n_latents=None, n_per_gif=15):
        """GIF of posterior traversals: rows are the latent dimensions, columns the images of data; frame j shows step j of
        every traversal.  All images go through ONE encoder pass and all their traversal latents through one decoder pass."""
        n_images, _, _, width_col = data.shape
        width_col = int(width_col * self.upsample_factor)
        n_latents = n_latents if n_latents is not None else self.model.latent_dim
        posts = self._posteriors(data)
        latents = torch.cat([self._traversal_latents(n_per_gif, post) for post in posts], dim=0)
        decoded = self._decode_latents(latents)
        per_image = decoded.shape[0] // n_images
        grids = [self._traversal_rows_grid(decoded[i * per_image:(i + 1) * per_image], n_per_gif, n_latents)
                 for i in range(n_images)]
        grids = torch.stack(grids).cpu().numpy()              # ONE device-to-host copy of every grid
        all_cols = [[] for _ in range(n_per_gif)]
        for grid in grids:
            height, width, c = grid.shape
            padding_width = (width - width_col * n_per_gif) // (n_per_gif + 1)
            for j in range(n_per_gif):
                x0 = (j + 1) * padding_width + j * width_col
                all_cols[j].append(grid[:, x0:x0 + width_col, :])
        pad_values = (1 - get_background(self.dataset)) * 255
        frames = [concatenate_pad(cols, pad_size=2, pad_values=pad_values, axis=1) for cols in all_cols]
        save_gif(os.path.join(self.model_dir, PLOT_NAMES["gif_traversals"]), frames)
        return frames

    def _traversal_rows_grid(self, decoded, n_per_latent, n_latents):
        decoded = self._reorder(decoded, n_per_latent)[:n_per_latent * n_latents]
        return self._grid(decoded, (n_latents, n_per_latent))


class GifTraversalsTraining:
    """GIF of prior traversals, one frame per training epoch (``Trainer(..., gif_visualizer=...)`` calls it after every epoch
    and ``save_reset()`` at the end; utils/visualize.py:364-432).

    A frame adds no host synchronisation: decoded and gridded on the device, its uint8 bytes are copied without blocking into
    pinned host memory behind an event; the frames become arrays in ``save_reset()``.  The training run is not disturbed: prior
    traversals draw no random numbers, train / eval mode is restored, and the passes run on a private engine
    (``_NativePasses``), so the workspaces and recorded launch plans of the training step stay as they were."""

    def __init__(self, model, dataset, model_dir, is_reorder_latents=False, n_per_latent=10, n_latents=None, **kwargs):
        self.save_filename = os.path.join(model_dir, GIF_FILE)
        self.visualizer = Visualizer(model, dataset, model_dir, save_images=False, **kwargs)
        self.images = []            # (pinned host uint8 [h, w, 3] tensor, event recorded behind its copy) per frame
        self.is_reorder_latents = is_reorder_latents
        self.n_per_latent = n_per_latent
        self.n_latents = n_latents if n_latents is not None else model.latent_dim

    def __call__(self):
        """Generate the next gif image. Should be called after each epoch."""
        model = self.visualizer.model
        cached_training = model.training
        model.eval()
        try:
            grid = self.visualizer._traversal_grid(None, self.is_reorder_latents, self.n_per_latent, self.n_latents)
            host = torch.empty(grid.shape, dtype=torch.uint8, pin_memory=True)
            host.copy_(grid, non_blocking=True)
            done = torch.cuda.Event()
            done.record()
            self.images.append((host, done))
        finally:
            if cached_training:
                model.train()

    def frames(self):
        """The frames so far as uint8 [h, w, 3] arrays (waits for their copies)."""
        out = []
        for host, done in self.images:
            done.synchronize()
            out.append(host.numpy())
        return out

    def save_reset(self):
        """Saves the GIF and resets the list of images. Call at the end of training."""
        frames = self.frames()
        if frames:
            save_gif(self.save_filename, frames, fps=FPS_GIF)
        self.images = []
