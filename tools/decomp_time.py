"""Cost of the joint log-density behind Evaluator.compute_elbo_decomposition (dvae_eval_joint_logq, csrc/elbo_decomp.hip) at
dSprites size, next to (a) the torch code a user would write without it -- chunked [S_chunk, N, D] log-densities + logsumexp on
the same GPU, the temporary sized to 2 GiB -- and (b) dvae_latent_entropy (the marginal entropies) at the same shape.

Device events around each call, `--reps` repeats after a warm-up, the median; inputs from a seed.  The torch baseline is timed on
its first `--torch-samples` samples and scaled to S where S is larger (its chunks are independent and equal): marked
"extrapolated".  Rates: (sample, data point, dim) triples per second over the D real dimensions, and as a share of the fp32 VALU
instruction rate / 3 (three VALU operations per triple; 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz = 39.3e12 lane-operations per
second, the unpacked quarter of the 157.3 TFLOPS vector peak).  Prints one JSON line per shape.

    python tools/decomp_time.py [--reps 5] [--torch-samples 10000]
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "disentangling-vae_amd")]

import torch  # noqa: E402

from disvae_amd import _evallib, _lib  # noqa: E402
from disvae_amd.engine import _stream  # noqa: E402

VALU_LANE_OPS_PER_S = 256 * 4 * 16 * 2.4e9
SHAPES = [(737280, 10, 10000), (737280, 10, 65536), (737280, 16, 10000)]
LOG2PI = math.log(2 * math.pi)


def median_ms(fn, reps):
    fn()                                                              # warm-up: code objects, allocator
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


def torch_joint_logq(z, mean, logvar, out, budget_bytes=2 << 30):
    N, D = mean.shape
    step = max(1, budget_bytes // (N * D * 4))
    c, iv = -0.5 * (LOG2PI + logvar), torch.exp(-logvar)
    for s0 in range(0, z.shape[0], step):
        ld = c[None] - 0.5 * (z[s0:s0 + step, None, :] - mean[None]) ** 2 * iv[None]
        out[s0:s0 + step] = torch.logsumexp(ld.sum(2), 1) - math.log(N)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torch-samples", type=int, default=10000)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is nothing to time without it"
    E, M = _evallib.lib(), _lib.lib()
    for N, D, S in SHAPES:
        gen = torch.Generator(device="cuda").manual_seed(N + D + S)
        centers = 2.0 * torch.randn(8, D, generator=gen, device="cuda")
        mean = 0.3 * torch.randn(N, D, generator=gen, device="cuda") + centers[torch.arange(N, device="cuda") % 8]
        logvar = -2.0 + 2.5 * torch.rand(N, D, generator=gen, device="cuda")
        rows = torch.randperm(N, generator=gen, device="cuda")[:S]
        z = (mean[rows] + torch.exp(0.5 * logvar[rows]) * torch.randn(S, D, generator=gen, device="cuda")).contiguous()
        ws = torch.empty(max(E.dvae_eval_joint_logq_ws_floats(N, D, S), M.dvae_latent_entropy_ws_floats(N, D, S)), device="cuda")
        logqz, H, Hd = torch.empty(S, device="cuda"), torch.empty(1, device="cuda"), torch.empty(D, device="cuda")
        z_ds = z.t().contiguous()
        st = _stream()
        joint = median_ms(lambda: _evallib.call("dvae_eval_joint_logq", z.data_ptr(), mean.data_ptr(), logvar.data_ptr(), N, D, S,
                                                ws.data_ptr(), logqz.data_ptr(), H.data_ptr(), st), args.reps)
        kernel_logqz = logqz.clone()
        marg = median_ms(lambda: _lib.call("dvae_latent_entropy", z_ds.data_ptr(), mean.data_ptr(), logvar.data_ptr(), N, D, S,
                                           ws.data_ptr(), Hd.data_ptr(), st), args.reps)
        St = min(S, args.torch_samples)
        ref = torch.empty(St, device="cuda")
        tor = median_ms(lambda: torch_joint_logq(z[:St], mean, logvar, ref), args.reps)
        scale = S / St
        triples = float(N) * D * S
        err = (kernel_logqz[:St] - ref).abs().max().item()
        print(json.dumps({
            "N": N, "D": D, "S": S, "reps": args.reps,
            "joint_logq_ms": round(joint[0], 3), "joint_logq_spread_ms": [round(joint[1], 3), round(joint[2], 3)],
            "latent_entropy_ms": round(marg[0], 3), "latent_entropy_spread_ms": [round(marg[1], 3), round(marg[2], 3)],
            "torch_chunked_ms": round(tor[0] * scale, 1), "torch_extrapolated": St < S, "torch_samples_timed": St,
            "torch_spread_ms": [round(tor[1] * scale, 1), round(tor[2] * scale, 1)],
            "speedup_vs_torch": round(tor[0] * scale / joint[0], 1),
            "joint_triples_per_s": round(triples / (joint[0] * 1e-3), -9),
            "joint_share_of_valu_rate_over_3": round(triples / (joint[0] * 1e-3) / (VALU_LANE_OPS_PER_S / 3), 3),
            "max_abs_diff_kernel_vs_torch_fp32": err, "H_joint": H.item()}), flush=True)
        del ws, mean, logvar, z, z_ds, ref
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
