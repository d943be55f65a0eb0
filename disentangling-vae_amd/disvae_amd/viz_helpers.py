"""Helpers of the native visualizer, with the names of utils/viz_helpers.py: the image grid of a decoded batch is built on the
device (dvae_image_grid_u8: F.interpolate(nearest) + make_grid + make_grid_img in one launch) and only its uint8 bytes cross to
the host.  No torchvision, imageio or pandas: images and GIFs are written with PIL, the loss log is read with ``csv``."""
import csv
import ctypes
import numbers

import numpy as np
import torch
from PIL import Image, ImageDraw

from . import _lib
from ._lib import call, ptr

FPS_GIF = 12

# utils/datasets.py: `background_color` of every dataset class (COLOUR_BLACK = 0, COLOUR_WHITE = 1).  A local table: that module
# needs torchvision.
BACKGROUNDS = {"mnist": 0, "fashion": 0, "dsprites": 0, "celeba": 1, "chairs": 1}


def get_background(dataset):
    """Background colour (0 black, 1 white) of a dataset (utils/datasets.py:44-46)."""
    try:
        return BACKGROUNDS[dataset.lower()]
    except KeyError:
        raise ValueError("Unkown dataset: {}".format(dataset))


def check_upsample(factor):
    """The nearest-neighbour upsampling factor: an integer >= 1 (main_viz.py parses it as an int)."""
    if isinstance(factor, bool) or not isinstance(factor, numbers.Integral) or factor < 1:
        raise ValueError("upsample_factor={!r}: expected an integer >= 1".format(factor))
    return int(factor)


def sort_list_by_other(to_sort, other, reverse=True):
    """Sort a list by an other."""
    return [el for _, el in sorted(zip(other, to_sort), reverse=reverse)]


def read_loss_from_file(log_file_path, loss_to_fetch):
    """Values of the losses named ``<loss_to_fetch><i>`` in the LAST epoch of an 'Epoch,Loss,Value' log, ordered by i (the
    per-dimension KL of the final epoch, for ``loss_to_fetch="kl_loss_"``)."""
    with open(log_file_path, newline="") as f:
        rows = list(csv.DictReader(f))
    if not rows:
        return []
    last = max(int(r["Epoch"]) for r in rows)
    picked = [(int(r["Loss"].replace(loss_to_fetch, "")), float(r["Value"]))
              for r in rows if int(r["Epoch"]) == last and r["Loss"].startswith(loss_to_fetch)]
    return [v for _, v in sorted(picked, key=lambda kv: kv[0])]


def add_labels(input_image, labels):
    """A copy of ``input_image`` (PIL) 100 pixels wider, one label per row band drawn in that margin (default font)."""
    new_width = input_image.width + 100
    new_img = Image.new("RGB", (new_width, input_image.height), color="white")
    new_img.paste(input_image, (0, 0))
    draw = ImageDraw.Draw(new_img)
    for i, s in enumerate(labels):
        draw.text(xy=(new_width - 100 + 0.005, int((i / len(labels) + 1 / (2 * len(labels))) * input_image.height)),
                  text=s, fill=(0, 0, 0))
    return new_img


def grid_shape(n, H, W, nrow=8, padding=2, upsample=1):
    """(height, width) of the grid of ``n`` H x W images (dvae_image_grid_shape: host only)."""
    h, w = ctypes.c_long(), ctypes.c_long()
    call("dvae_image_grid_shape", int(n), int(H), int(W), int(nrow), int(padding), int(upsample), ctypes.addressof(h),
         ctypes.addressof(w))
    return h.value, w.value


def to_f32_device(images, device):
    """An NCHW batch as contiguous fp32 on ``device``: fp32 images as they are, uint8 pixels through dvae_u8_to_f32 (ToTensor's
    float(v) / 255, bit for bit)."""
    x = images.to(device, non_blocking=True)
    if x.dtype == torch.uint8:
        x = x.contiguous()
        if x.data_ptr() % 16:
            x = x.clone()
        out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        call("dvae_u8_to_f32", ptr(x), ptr(out), x.numel(), torch.cuda.current_stream(x.device).cuda_stream)
        return out
    if x.dtype != torch.float32:
        raise TypeError("images must be float32 in [0, 1] or uint8 pixels, got %s" % x.dtype)
    return x.contiguous()


def image_grid_u8(images, nrow=8, padding=2, pad_value=0., upsample=1, out=None):
    """uint8 [h, w, 3] DEVICE tensor: the grid that ``make_grid_img(F.interpolate(images, scale_factor=upsample), nrow=nrow,
    padding=padding, pad_value=pad_value)`` returns, in one launch (dvae_image_grid_u8).  ``images``: [n, C, H, W], C = 1 or 3,
    on the device (fp32, or uint8 pixels)."""
    if images.dim() != 4 or images.shape[1] not in (1, 3):
        raise ValueError("expected an [n, C, H, W] batch with C = 1 or 3, got shape {}".format(tuple(images.shape)))
    upsample = check_upsample(upsample)
    if images.device.type != "cuda":
        raise _lib.DvaeHipError("image_grid_u8 runs on the device: images are on %s" % images.device)
    x = to_f32_device(images, images.device)
    n, C, H, W = x.shape
    h, w = grid_shape(n, H, W, nrow, padding, upsample)
    if out is None:
        out = torch.empty((h, w, 3), dtype=torch.uint8, device=x.device)
    elif out.shape != (h, w, 3) or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != x.device:
        raise ValueError("out must be a contiguous uint8 [%d, %d, 3] tensor on %s" % (h, w, x.device))
    call("dvae_image_grid_u8", ptr(x), n, C, H, W, int(nrow), int(padding), float(pad_value), upsample, ptr(out),
         torch.cuda.current_stream(x.device).cuda_stream)
    return out


def make_grid_img(tensor, nrow=8, padding=2, pad_value=0., upsample=1):
    """The grid of ``image_grid_u8`` as a host uint8 [h, w, 3] array (one device-to-host copy, of the uint8 bytes)."""
    return image_grid_u8(tensor, nrow, padding, pad_value, upsample).cpu().numpy()


def concatenate_pad(arrays, pad_size, pad_values, axis=0):
    """Concatenate a list of arrays along ``axis`` with ``pad_size`` slices of ``pad_values`` before, between and after them."""
    pad = np.ones_like(arrays[0]).take(indices=range(pad_size), axis=axis) * pad_values
    new_arrays = [pad]
    for arr in arrays:
        new_arrays += [arr, pad]
    new_arrays += [pad]
    return np.concatenate(new_arrays, axis=axis)


def save_png(img, filename):
    """Write a uint8 [h, w, 3] array as PNG (what save_image writes)."""
    Image.fromarray(np.ascontiguousarray(img)).save(filename)


def save_gif(filename, frames, fps=FPS_GIF):
    """Write uint8 [h, w, 3] frames as a looping GIF.  Grey frames (R = G = B, every 1-channel dataset) are stored as 8-bit grey
    and decode back exactly; colour frames go through PIL's palette quantisation."""
    frames = [np.ascontiguousarray(f) for f in frames]
    grey = all(np.array_equal(f[..., 0], f[..., 1]) and np.array_equal(f[..., 0], f[..., 2]) for f in frames)
    ims = [Image.fromarray(f[..., 0] if grey else f) for f in frames]
    ims[0].save(filename, save_all=True, append_images=ims[1:], duration=round(1000 / fps), loop=0)
