"""Per-image scores of a native VAE (new: the reference reports batch means of the ELBO terms only).

* ``per_image_losses``: the reconstruction term and the per-dimension KL of every image under the eval-mode forward (z = mean,
  vae.py:69-71) -- the values whose means over a data set are the Evaluator's ``recon_loss`` and ``kl_loss_<d>`` of the VAE loss.
* ``log_likelihood``: the importance-weighted bound of Burda et al. (IWAE),
      log p(x) ~ logsumexp_k [log p(x|z_k) + log p(z_k) - log q(z_k|x)] - log K,   z_k ~ q(z|x),
  with log p(x|z) = -(the reconstruction term of losses.py:394-449).  For bernoulli that term IS -log p(x|z) and the estimate is
  the IWAE bound on log p(x) in nats.  For gaussian and laplace the reference's loss leaves out the likelihood's normalising
  constant (and scales it), so the value is the bound only up to that constant -- fine for ranking images or comparing models
  with the same rec_dist, not as an absolute log-likelihood.

Every image is encoded once; its K samples are reparameterised (dvae_reparam_kl_fwd), decoded in passes of at most
``_ScorePasses.MAX_ROWS`` rows, scored row by row against the image (dvae_recon_rows: every target quad is loaded once per
workgroup and reused from registers for 8 reconstruction rows) and folded into a running logsumexp per image (dvae_iw_loglik),
so one image's samples may span several passes.  The passes run on a PRIVATE engine over the model's parameters (visualize._NativePasses): the model's
own engine keeps its workspaces and the launch plans its training step recorded.  The N(0, 1) draws come from a private
``torch.Generator`` or from the caller (``eps``): the global CPU and device random states are not touched.
"""
import contextlib
import ctypes

import torch

from . import _lib
from ._lib import call, ptr
from .engine import _stream
from .visualize import _NativePasses, _private_allocs
from .viz_helpers import to_f32_device


def check_rec_dist(rec_dist):
    if rec_dist not in _lib.REC:
        raise ValueError("Unkown distribution: {}".format(rec_dist))      # (losses.py:442's message)
    return _lib.REC[rec_dist]


def plan_passes(n_img, n_samples, rows):
    """Decoder passes of the estimate as (i0, i1, k0, k1): images [i0, i1), samples [k0, k1) of each.  max(1, rows // K) whole
    images per pass while K <= rows; above, every image alone in ceil(K / rows) passes of at most `rows` samples."""
    if n_samples <= rows:
        per = max(1, rows // n_samples)
        return [(i0, min(n_img, i0 + per), 0, n_samples) for i0 in range(0, n_img, per)]
    return [(i, i + 1, k0, min(n_samples, k0 + rows)) for i in range(n_img) for k0 in range(0, n_samples, rows)]


class _ScorePasses(_NativePasses):
    """The model's private engine for the scores (one per model, kept on it: its workspace is reused from batch to batch)."""

    @classmethod
    def of(cls, model):
        p = model.__dict__.get("_score_passes")
        if p is None:
            p = model.__dict__["_score_passes"] = cls(model)
        return p

    def recon_rows(self, recon, target, n_img, K, dist, out):
        """dvae_recon_rows of n_img images x K rows of `recon` into out[:n_img * K], with its workspace (kept, grown)."""
        row = target[0].numel()
        need = ctypes.c_long()
        call("dvae_recon_rows_ws_floats", n_img, K, row, ctypes.addressof(need))
        ws = self.__dict__.get("_rows_ws")
        if need.value and (ws is None or ws.numel() < need.value or ws.device != recon.device):
            ws = self._rows_ws = torch.empty(need.value, dtype=torch.float32, device=recon.device)
        call("dvae_recon_rows", ptr(recon), ptr(target), int(target.dtype == torch.uint8), n_img, K, row, dist,
             ptr(ws) if need.value else None, ptr(out), _stream())


@contextlib.contextmanager
def _eval_mode(model):
    was = model.training
    model.eval()
    try:
        yield
    finally:
        if was:
            model.train()


def _images(model, x):
    """The batch on the model's device: (fp32 images for the encoder, the target as given -- fp32 or uint8 -- contiguous)."""
    if x.dim() != 4 or tuple(x.shape[1:]) != tuple(model.img_size):
        raise ValueError("expected a batch of shape [N, %s], got %s" % (", ".join(str(v) for v in model.img_size), tuple(x.shape)))
    if x.dtype not in (torch.float32, torch.uint8):
        raise TypeError("images must be float32 in [0, 1] or uint8 pixels, got %s" % x.dtype)
    dev = model.arena.flat.device
    target = x.to(dev).contiguous()
    if target.data_ptr() % 16:                        # (a view at an offset: the kernels read 16-byte aligned rows)
        target = target.clone()
    return to_f32_device(target, dev), target


def per_image_losses(model, x, rec_dist="bernoulli"):
    """{"recon": [N], "kl": [N, D]} (fp32, on the device) of the batch x ([N, C, H, W], fp32 in [0, 1] or uint8 pixels) under
    the eval-mode forward (z = mean): recon[i] = the reconstruction term of losses.py:394-449 of image i alone, kl[i, d] =
    0.5 (-1 - logvar + mean^2 + e^logvar).  Their means over the images are the ``recon_loss`` / ``kl_loss_<d>`` that
    Evaluator.compute_losses reports for the VAE loss."""
    dist = check_rec_dist(rec_dist)
    passes = _ScorePasses.of(model)
    passes.check_device()
    with _eval_mode(model):
        xf, target = _images(model, x)
        N, D = xf.shape[0], model.latent_dim
        rec = torch.empty(N, dtype=torch.float32, device=xf.device)
        kl = torch.empty(N, D, dtype=torch.float32, device=xf.device)
        mu, logvar = passes.encode(xf)
        with _private_allocs():
            eng, buf = passes._buffers(min(N, passes.MAX_ROWS))
            eng.stage()
            s = _stream()
            for lo in range(0, N, passes.MAX_ROWS):
                hi = min(N, lo + passes.MAX_ROWS)
                eng.decode(mu[lo:hi], buf, n=hi - lo, staged=True)
                passes.recon_rows(buf.recon, target[lo:hi], hi - lo, 1, dist, rec[lo:hi])
            call("dvae_iw_loglik", ptr(mu), ptr(logvar), None, None, None, N, 1, D, 1, 1, 1, None, None, ptr(kl), s)
    return {"recon": rec, "kl": kl}


def _draws(eps, N, K, D, dev):
    if eps.shape not in ((N, K, D), (N * K, D)):
        raise ValueError("eps must have shape [%d, %d, %d] (or [%d, %d]), got %s" % (N, K, D, N * K, D, tuple(eps.shape)))
    return eps.to(dev, torch.float32).reshape(N * K, D).contiguous()


def log_likelihood(model, x, n_samples=128, rec_dist="bernoulli", generator=None, eps=None):
    """Importance-weighted estimate of log p(x) per image (nats, [N] fp32 on the device) with K = n_samples samples of q(z|x)
    each -- exact bound for bernoulli, up to the missing normalising constant for gaussian / laplace (module docstring).
    x: [N, C, H, W] fp32 in [0, 1] or uint8 pixels.  The draws: eps ([N, K, D] or [N*K, D], image-major), else N(0, 1) from
    `generator` (a torch.Generator on the CPU or the device; default: a private one seeded with 0) in pass order."""
    K = int(n_samples)
    if K < 1:
        raise ValueError("n_samples must be >= 1, got %r" % (n_samples,))
    dist = check_rec_dist(rec_dist)
    passes = _ScorePasses.of(model)
    dev = passes.check_device()
    with _eval_mode(model):
        xf, target = _images(model, x)
        N, D = xf.shape[0], model.latent_dim
        if eps is not None:
            eps = _draws(eps, N, K, D, dev)
        elif generator is None:
            generator = torch.Generator(device=dev).manual_seed(0)
        R = passes.MAX_ROWS
        plan = plan_passes(N, K, R)
        out = torch.empty(N, dtype=torch.float32, device=dev)
        mu, logvar = passes.encode(xf)
        ml = torch.stack((mu, logvar), dim=-1).reshape(N, 2 * D)        # mu_logvar_gen's interleaved layout
        with _private_allocs():
            eng, buf = passes._buffers(min(R, N * K))
            per = max(i1 - i0 for i0, i1, _, _ in plan)
            state = torch.empty(per, 2, dtype=torch.float32, device=dev)
            rec = torch.empty(R, dtype=torch.float32, device=dev)
            eng.stage()
            s = _stream()
            for i0, i1, k0, k1 in plan:
                n, nk = i1 - i0, k1 - k0
                rows = n * nk
                buf.ml[:rows].view(n, nk, 2 * D).copy_(ml[i0:i1].unsqueeze(1).expand(n, nk, 2 * D))
                if eps is not None:
                    e = eps.view(N, K, D)[i0:i1, k0:k1].reshape(rows, D)
                else:
                    e = torch.randn((rows, D), generator=generator, device=generator.device, dtype=torch.float32)
                e = e.to(dev).contiguous()
                eng.reparam(buf, e, n=rows)                                 # z = mu + exp(logvar / 2) eps: the decoder's input
                eng.decode(buf.z, buf, n=rows, staged=True)
                passes.recon_rows(buf.recon, target[i0:i1], n, nk, dist, rec)
                call("dvae_iw_loglik", ptr(mu[i0:i1]), ptr(logvar[i0:i1]), ptr(buf.z), ptr(e), ptr(rec), n, nk, D, K,
                     int(k0 == 0), int(k1 == K), ptr(state), ptr(out[i0:i1]), None, s)
    return out
