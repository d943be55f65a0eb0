"""Cost of the interventional-robustness kernels (libdvae_irs_hip.so, csrc/factor_irs.hip) and of the whole irs_from_table at
dSprites size (N = 737 280, D = 10, lat_sizes (3, 6, 40, 32, 32)), with all rows and with a 10 000-row draw, with the default 20
factor bins and with every value its own group, next to the torch code a user would write without them on the same GPU: per
group a boolean mask, the mean, the absolute deviations and torch.quantile -- batched on the device, one copy at the end.

Two tables: "gauss" (independent Gaussian columns) and "disentangled" (column d follows factor d % 5 plus 1e-3 noise: the
deviations of a group share their leading digits).  Device events around each call, `--reps` repeats after a warm-up, the median
and the spread; inputs from a seed.  The scores of both versions are compared before timing.  Prints one JSON line per
measurement and writes them to --out.

    python tools/irs_time.py [--reps 20] [--out profiles/irs_time.jsonl]
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

from disvae_amd import _irslib  # noqa: E402
from disvae_amd.engine import _stream  # noqa: E402
from disvae_amd.evaluate import irs_from_table, irs_group_map, irs_quantile_ranks  # noqa: E402

LAT = (3, 6, 40, 32, 32)
N, D, K, Q = 737280, 10, 5, 0.99


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "irs_time.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is nothing to time without it"
    lines = []

    def emit(what, t, **more):
        lines.append(json.dumps(dict({"what": what, "N": N, "D": D, "K": K, "diff_quantile": Q, "reps": args.reps, "median_ms": t[0],
                                      "spread_ms": t[1]}, **more)))
        print(lines[-1], flush=True)

    gen = torch.Generator(device="cuda").manual_seed(1)
    strides = [int(np.prod(LAT[k + 1:])) for k in range(K)]
    r = torch.arange(N, device="cuda")
    values = torch.stack([(r // strides[k]) % LAT[k] for k in range(K)], dim=1)                     # [N, K] int64, for torch only
    tables = {"gauss": torch.randn(N, D, generator=gen, device="cuda").contiguous(),
              "disentangled": (values[:, torch.arange(D) % K].float() + 1e-3 * torch.randn(N, D, generator=gen, device="cuda")).contiguous()}
    draw = torch.randperm(N, generator=gen, device="cuda")[:10000].contiguous()
    sizes = torch.tensor(LAT, dtype=torch.int32, device="cuda")
    h = _irslib.lib()
    st = _stream()
    for bins in (20, None):
        gmap, n_groups = irs_group_map(LAT, bins)
        total, most = 1 + sum(n_groups), max(n_groups)
        gmap_dev, groups_dev = torch.from_numpy(gmap).cuda(), torch.tensor(n_groups, dtype=torch.int32, device="cuda")
        offsets = np.concatenate([[0], np.cumsum(LAT)])
        gid = torch.stack([gmap_dev[int(offsets[k]) + values[:, k]].long() for k in range(K)], dim=1)   # [N, K], for torch only
        for name, table in tables.items():
            for sel, rows in (("all rows", None), ("10000 drawn rows", draw)):
                S = N if rows is None else int(rows.numel())
                layout = (N, D, K, S, sum(LAT), total, most)
                ws = torch.empty(max(h.dvae_irs_group_means_ws_floats(N, D, K, S, total),
                                     h.dvae_irs_group_order_stats_ws_floats(N, D, K, S, total)), device="cuda")
                counts = torch.empty(total, dtype=torch.int32, device="cuda")
                means = torch.empty(total, D, device="cuda")
                stats = torch.empty(3, total, D, device="cuda")
                ptrs = (table.data_ptr(), None if rows is None else rows.data_ptr(), sizes.data_ptr(), gmap_dev.data_ptr(),
                        groups_dev.data_ptr())

                def group_means():
                    _irslib.call("dvae_irs_group_means", *ptrs, *layout, ws.data_ptr(), counts.data_ptr(), means.data_ptr(), st)
                group_means()
                rank = irs_quantile_ranks(counts.cpu().numpy(), Q)[0]
                rank[0] = S - 1
                rank_dev = torch.from_numpy(rank.astype(np.int32)).cuda()

                def order_stats():
                    _irslib.call("dvae_irs_group_order_stats", *ptrs, means.data_ptr(), rank_dev.data_ptr(), *layout, ws.data_ptr(),
                                 stats[0].data_ptr(), stats[1].data_ptr(), stats[2].data_ptr(), st)

                def torch_irs():
                    x = table if rows is None else table[rows]
                    g = gid if rows is None else gid[rows]
                    max_dev = (x - x.mean(0)).abs().amax(0)
                    matrix = []
                    for k in range(K):
                        diffs = []
                        for u in range(n_groups[k]):
                            xs = x[g[:, k] == u]
                            if xs.shape[0]:
                                diffs.append(torch.quantile((xs - xs.mean(0)).abs(), Q, dim=0))
                        matrix.append(1.0 - torch.stack(diffs).mean(0) / max_dev)
                    matrix = torch.stack(matrix, dim=1)
                    return (matrix.amax(1) * max_dev).sum() / max_dev.sum()

                ours = irs_from_table(table, LAT, diff_quantile=Q, factor_bins=bins, rows=rows)["IRS"]
                theirs = float(torch_irs())
                assert abs(ours - theirs) < 1e-3, (ours, theirs)      # (torch: fp32 means and quantiles)
                more = dict(table=name, rows=sel, S=S, factor_bins=bins, total_groups=total)
                t_means, t_stats = median_ms(group_means, args.reps), median_ms(order_stats, args.reps)
                emit("dvae_irs_group_means", t_means, **more)
                emit("dvae_irs_group_order_stats", t_stats, **more)
                t_torch = median_ms(torch_irs, max(args.reps // 4, 3))
                emit("torch: per group a mask, mean, |x - mean| and torch.quantile", t_torch,
                     **dict(more, irs_native=ours, irs_torch=theirs, torch_over_both_launches=round(t_torch[0] / (t_means[0] + t_stats[0]), 2)))

                def whole():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    irs_from_table(table, LAT, diff_quantile=Q, factor_bins=bins, rows=rows)
                    torch.cuda.synchronize()
                    return (time.perf_counter() - t0) * 1e3
                whole()
                w = sorted(whole() for _ in range(5))
                emit("irs_from_table (both launches, two copies, the host's fp64), wall clock",
                     (round(w[2], 2), [round(w[0], 2), round(w[4], 2)]), **more)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
