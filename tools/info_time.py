"""Cost of the information-score kernels (libdvae_info_hip.so, csrc/factor_info.hip) and of the whole
information_scores_from_table at dSprites size (N = 737 280, D = 10, lat_sizes (3, 6, 40, 32, 32), 20 bins), next to the torch
code a user would write without them on the same GPU: one bucketize + bincount per (latent, factor) pair with a materialised
index -- 50 pairs, batched on the device, no copy in between -- and torch's min / max / cov for the moments.

Two tables: "gauss" (independent Gaussian columns: the adds of a wave spread over the bins) and "disentangled" (column d follows
factor d % 5 plus 1e-3 noise: 64 consecutive rows of a slow factor fall into one bin).  Device events around each call, `--reps`
repeats after a warm-up, the median and the spread; inputs from a seed.  The counts of both versions are compared before timing.
Prints one JSON line per measurement and writes them to --out.

    python tools/info_time.py [--reps 20] [--out profiles/factor_info_time.jsonl]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "disentangling-vae_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from disvae_amd import _infolib  # noqa: E402
from disvae_amd.engine import _stream  # noqa: E402
from disvae_amd.evaluate import histogram_edges, information_scores_from_table  # noqa: E402

LAT = (3, 6, 40, 32, 32)
N, D, K, BINS = 737280, 10, 5, 20


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
    return round(times[len(times) // 2], 4), [round(times[0], 4), round(times[-1], 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "factor_info_time.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is nothing to time without it"
    lines = []

    def emit(what, t, **more):
        lines.append(json.dumps(dict({"what": what, "N": N, "D": D, "K": K, "n_bins": BINS, "reps": args.reps, "median_ms": t[0],
                                      "spread_ms": t[1]}, **more)))
        print(lines[-1], flush=True)

    gen = torch.Generator(device="cuda").manual_seed(1)
    strides = [int(np.prod(LAT[k + 1:])) for k in range(K)]
    r = torch.arange(N, device="cuda")
    values = torch.stack([(r // strides[k]) % LAT[k] for k in range(K)], dim=1)                     # [N, K] int64, for torch only
    tables = {"gauss": torch.randn(N, D, generator=gen, device="cuda").contiguous(),
              "disentangled": (values[:, torch.arange(D) % K].float() + 1e-3 * torch.randn(N, D, generator=gen, device="cuda")).contiguous()}
    sizes = torch.tensor(LAT, dtype=torch.int32, device="cuda")
    total = sum(LAT)
    h = _infolib.lib()
    ws = torch.empty(max(h.dvae_info_moments_ws_floats(N, D, K, N), 1), device="cuda")
    mom = [torch.empty(n, device="cuda") for n in (D, D, D, D, D * K, K, K)]
    counts = torch.empty(D, BINS * total, dtype=torch.int32, device="cuda")
    st = _stream()
    for name, table in tables.items():
        def moments():
            _infolib.call("dvae_info_moments", table.data_ptr(), None, sizes.data_ptr(), N, D, K, N, ws.data_ptr(),
                          *[m.data_ptr() for m in mom], st)
        moments()
        lo, hi = mom[0].cpu().numpy(), mom[1].cpu().numpy()
        edges = torch.from_numpy(np.stack([histogram_edges(lo[d], hi[d], BINS) for d in range(D)])).cuda()

        def hist():
            _infolib.call("dvae_info_joint_hist", table.data_ptr(), None, sizes.data_ptr(), edges.data_ptr(), N, D, K, N, BINS, total,
                          None, counts.data_ptr(), st)

        def torch_hist():
            out = []
            for d in range(D):
                b = (torch.bucketize(table[:, d], edges[d], right=True) - 1).clamp_(0, BINS - 1)
                for k in range(K):
                    out.append(torch.bincount(b * LAT[k] + values[:, k], minlength=BINS * LAT[k]))
            return out

        def torch_moments():
            x = torch.cat([table, values.float()], dim=1)
            return table.min(0).values, table.max(0).values, x.mean(0), torch.cov(x.t())

        hist()
        ref = torch.cat([torch.cat(torch_hist()[d * K:(d + 1) * K]) for d in range(D)]).view(D, -1)
        same = bool((ref == counts.long()).all())
        assert same, "the kernel's counts differ from torch's"
        emit("dvae_info_moments, %s" % name, median_ms(moments, args.reps), table_bytes=N * D * 4)
        emit("dvae_info_joint_hist, %s" % name, median_ms(hist, args.reps), table_bytes=N * D * 4, counts_equal_torch=same)
        emit("torch: 50 x (bucketize + bincount) on a materialised index, %s" % name, median_ms(torch_hist, args.reps))
        emit("torch: min, max, mean, cov of [table | factor values], %s" % name, median_ms(torch_moments, args.reps))

        def whole():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            information_scores_from_table(table, LAT)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3
        whole()
        w = sorted(whole() for _ in range(5))
        emit("information_scores_from_table (both launches, two copies, the host's fp64), wall clock, %s" % name,
             (round(w[2], 2), [round(w[0], 2), round(w[4], 2)]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
