"""Cost of the label-free score kernels (libdvae_unsup_hip.so, csrc/latent_pairs.hip) and of the whole
unsupervised_scores_from_table at the dSprites shape (N = 737 280, D = 10, 20 bins) -- all rows, and 10 000 drawn rows -- next to
the torch code a user would write without them on the same GPU: torch.cov on the fp64 table (with min and max) for the moments,
and one bucketize pair + bincount for each of the 45 pairs of latents, batched on the device, no copy in between.

Three tables: "gauss" (independent Gaussian columns), "collapsed" (7 of the 10 columns at std 1e-3 around a constant, as the
unused dimensions of a trained VAE) and "disentangled" (column d follows factor d % 5 of the dSprites grid plus 1e-3 noise: 64
consecutive rows fall into one cell of most pairs, the case of the wave-uniform add).  Device events around each call, `--reps`
repeats after a warm-up, the median and the spread; inputs from a seed.  The counts and the covariance of both versions are
compared before timing.  Prints one JSON line per measurement and writes them to --out.

    python tools/unsup_time.py [--reps 20] [--out profiles/unsup_time.jsonl]
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

from disvae_amd import _unsuplib  # noqa: E402
from disvae_amd.engine import _stream  # noqa: E402
from disvae_amd.evaluate import histogram_edges, unsupervised_scores_from_table  # noqa: E402

LAT = (3, 6, 40, 32, 32)
N, D, BINS, DRAWN = 737280, 10, 20, 10000
PAIRS = [(d, e) for d in range(D) for e in range(d + 1, D)]


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unsup_time.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is nothing to time without it"
    lines = []

    def emit(what, t, **more):
        lines.append(json.dumps(dict({"what": what, "N": N, "D": D, "n_bins": BINS, "reps": args.reps, "median_ms": t[0],
                                      "spread_ms": t[1]}, **more)))
        print(lines[-1], flush=True)

    gen = torch.Generator(device="cuda").manual_seed(1)
    strides = [int(np.prod(LAT[k + 1:])) for k in range(len(LAT))]
    r = torch.arange(N, device="cuda")
    values = torch.stack([(r // strides[k]) % LAT[k] for k in range(len(LAT))], dim=1)             # [N, 5] int64
    gauss = torch.randn(N, D, generator=gen, device="cuda")
    collapsed = gauss.clone()
    collapsed[:, 3:] = torch.linspace(-1, 1, 7, device="cuda") + 1e-3 * collapsed[:, 3:]
    tables = {"gauss": gauss.contiguous(), "collapsed": collapsed.contiguous(),
              "disentangled": (values[:, torch.arange(D) % len(LAT)].float() + 1e-3 * torch.randn(N, D, generator=gen, device="cuda")).contiguous()}
    drawn = torch.randperm(N, generator=gen, device="cuda")[:DRAWN].contiguous()
    h = _unsuplib.lib()
    ws = torch.empty(max(h.dvae_unsup_moments_ws_floats(N, D, N), 1), device="cuda")
    col_min, col_max = torch.empty(D, device="cuda"), torch.empty(D, device="cuda")
    col_mean, cov = torch.empty(D, dtype=torch.float64, device="cuda"), torch.empty(D, D, dtype=torch.float64, device="cuda")
    counts = torch.empty(len(PAIRS), BINS, BINS, dtype=torch.int32, device="cuda")
    st = _stream()
    for name, table in tables.items():
        for rows, S, sel in ((None, N, "all rows"), (drawn, DRAWN, "%d drawn rows" % DRAWN)):
            rp = None if rows is None else rows.data_ptr()
            picked = table if rows is None else table[rows]

            def moments():
                _unsuplib.call("dvae_unsup_moments", table.data_ptr(), rp, N, D, S, ws.data_ptr(), col_min.data_ptr(), col_max.data_ptr(),
                               col_mean.data_ptr(), cov.data_ptr(), st)
            moments()
            lo, hi = col_min.cpu().numpy(), col_max.cpu().numpy()
            edges = torch.from_numpy(np.stack([histogram_edges(lo[d], hi[d], BINS) for d in range(D)])).cuda()

            def hist():
                _unsuplib.call("dvae_unsup_pair_hist", table.data_ptr(), rp, edges.data_ptr(), N, D, S, BINS, None, counts.data_ptr(), st)

            def torch_hist():
                out = []
                for d, e in PAIRS:                                                            # a bucketize pair + a bincount
                    bd = (torch.bucketize(picked[:, d], edges[d], right=True) - 1).clamp_(0, BINS - 1)
                    be = (torch.bucketize(picked[:, e], edges[e], right=True) - 1).clamp_(0, BINS - 1)
                    out.append(torch.bincount(bd * BINS + be, minlength=BINS * BINS))
                return out

            def torch_moments():
                x = picked.double()
                return x.min(0).values, x.max(0).values, x.mean(0), torch.cov(x.t())

            hist()
            same = bool((torch.stack(torch_hist()).view(len(PAIRS), BINS, BINS) == counts.long()).all())
            assert same, "the kernel's counts differ from torch's"
            ref_cov = torch_moments()[3]
            cov_err = float(((cov - ref_cov).abs() / ref_cov.diag().sqrt().outer(ref_cov.diag().sqrt())).max())
            assert cov_err < 1e-9, cov_err
            more = dict(table=name, rows=sel, S=S)
            emit("dvae_unsup_moments", median_ms(moments, args.reps), table_bytes=N * D * 4, cov_vs_torch_rel=cov_err, **more)
            emit("dvae_unsup_pair_hist", median_ms(hist, args.reps), table_bytes=N * D * 4, counts_equal_torch=same, **more)
            emit("torch: min, max, mean, cov of the fp64 table", median_ms(torch_moments, args.reps), **more)
            emit("torch: 45 x (bucketize pair + bincount)", median_ms(torch_hist, args.reps), **more)

            def whole():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                unsupervised_scores_from_table(table, rows=rows)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3
            whole()
            w = sorted(whole() for _ in range(5))
            emit("unsupervised_scores_from_table (both launches, two copies, the host's fp64), wall clock",
                 (round(w[2], 2), [round(w[0], 2), round(w[4], 2)]), **more)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
