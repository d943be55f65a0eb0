"""Cost of the per-image scores (disvae_amd/likelihood.py): log_likelihood at K samples per image -- wall time and decoded rows
per second -- and the dvae_recon_rows kernel alone, as bytes per second and as a fraction of the ~6.3 TB/s an MI355X streams
(MI355X float4 copy).  Bytes counted: every reconstruction row once plus every target row once (the least the kernel must read).
"recon_rows_pass" is the operating point of log_likelihood (one pass of the private engine's 256 rows: 2 images x 128 samples);
"recon_rows_large" a call of 64 images x K rows, for comparison.
Geometries 64x64x3 and 32x32x1, fp32 targets.  Prints one JSON line.

    python tools/loglik_time.py [--images 256] [--samples 128] [--reps 5]
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "disentangling-vae_amd")]

import torch  # noqa: E402

from disvae_amd import _lib, init_specific_model, log_likelihood  # noqa: E402
from disvae_amd.engine import _stream  # noqa: E402
from disvae_amd.likelihood import _ScorePasses  # noqa: E402

HBM_BYTES_PER_S = 6.3e12


def recon_rows_rate(img, n_img, K, reps):
    """Kernel time of dvae_recon_rows over n_img images x K rows (events around `reps` back-to-back launches)."""
    row = img[0] * img[1] * img[2]
    gen = torch.Generator(device="cuda").manual_seed(0)
    recon = torch.rand((n_img * K, row), generator=gen, device="cuda")
    target = torch.rand((n_img, row), generator=gen, device="cuda")
    out = torch.empty(n_img * K, device="cuda")
    need = ctypes.c_long()
    _lib.call("dvae_recon_rows_ws_floats", n_img, K, row, ctypes.addressof(need))
    ws = torch.empty(max(1, need.value), device="cuda")
    args = (recon.data_ptr(), target.data_ptr(), 0, n_img, K, row, _lib.REC["bernoulli"], ws.data_ptr() if need.value else None,
            out.data_ptr(), _stream())
    for _ in range(3):
        _lib.call("dvae_recon_rows", *args)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        _lib.call("dvae_recon_rows", *args)
    e1.record()
    e1.synchronize()
    sec = e0.elapsed_time(e1) / 1e3 / reps
    nbytes = 4 * row * (n_img * K + n_img)
    return dict(rows=n_img * K, us=round(sec * 1e6, 2), GBps=round(nbytes / sec / 1e9, 1),
                frac_of_6p3TBps=round(nbytes / sec / HBM_BYTES_PER_S, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--samples", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    K, N = args.samples, args.images
    out = {"K": K, "images": N, "pass_rows": _ScorePasses.MAX_ROWS}
    for img in ((3, 64, 64), (1, 32, 32)):
        key = "x".join(str(v) for v in img[1:]) + "x%d" % img[0]
        torch.manual_seed(0)
        model = init_specific_model("Burgess", img, 10).to("cuda").eval()
        x = (torch.rand((N,) + img, generator=torch.Generator().manual_seed(1)) * 255).to(torch.uint8).to("cuda")
        log_likelihood(model, x[:8], n_samples=K)                        # warm-up: workspace, code objects
        torch.cuda.synchronize()
        walls = []
        for r in range(args.reps):
            g = torch.Generator(device="cuda").manual_seed(r)
            t = time.perf_counter()
            ll = log_likelihood(model, x, n_samples=K, generator=g)
            torch.cuda.synchronize()
            walls.append(time.perf_counter() - t)
        assert torch.isfinite(ll).all()
        wall = sorted(walls)[len(walls) // 2]
        out[key] = dict(log_likelihood_s=round(wall, 4), ms_per_image=round(wall / N * 1e3, 3),
                        decoded_rows_per_s=round(N * K / wall), spread_s=[round(min(walls), 4), round(max(walls), 4)],
                        recon_rows_pass=recon_rows_rate(img, _ScorePasses.MAX_ROWS // K or 1, min(K, _ScorePasses.MAX_ROWS),
                                                        200),
                        recon_rows_large=recon_rows_rate(img, 64, K, 50))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
