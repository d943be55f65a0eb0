"""Cost of the posterior mass table behind Evaluator.compute_interpretability_scores (dvae_mass_joint, csrc/posterior_mass.hip) at
the dSprites shape (N = 737 280 rows, lat_sizes (3, 6, 40, 32, 32), D = 10, 100 bins) over every row and over 10 000 drawn rows, on
three tables -- Gaussian means and log-variances; sharp, factor-aligned posteriors; 7 of the 10 columns collapsed to the prior --
next to what computes the same without it:
  (a) the torch code a user would write on the same GPU: chunks of rows, the [chunk, D, n_bins] fp64 bin masses by the same
      tail differences, one index_add_ per factor;
  (b) the whole interpretability_scores_from_table call (host clock, ends in the device->host copy and the fp64 scores).
--bench also runs `python bench.py` in a process of its own and records its result line: training does not load this library.

Device events around each call, `--reps` repeats after a warm-up, the median and the spread; inputs from a seed.  One JSON line
per (table, selection) is printed and appended to --out (profiles/mass_time.jsonl).

    python tools/mass_time.py [--reps 5] [--bench] [--out profiles/mass_time.jsonl]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "disentangling-vae_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from disvae_amd import _masslib, interpretability_scores_from_table  # noqa: E402
from disvae_amd.engine import _stream  # noqa: E402
from disvae_amd.evaluate import mass_edges  # noqa: E402

LAT_SIZES, D, N_BINS = (3, 6, 40, 32, 32), 10, 100
TABLES = ("gaussian", "sharp_aligned", "collapsed_7_of_10")


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


def factor_values(rows, lat_sizes):
    out, stride = [], 1
    for size in reversed(lat_sizes):
        out.append((rows // stride) % size)
        stride *= size
    return out[::-1]


def make_table(kind, N, gen):
    mean = torch.randn(N, D, generator=gen, device="cuda")
    logvar = -2.0 + 2.5 * torch.rand(N, D, generator=gen, device="cuda")
    if kind == "sharp_aligned":                                       # latent k holds factor k, the other five are noise
        v = factor_values(torch.arange(N, device="cuda"), LAT_SIZES)
        for k, size in enumerate(LAT_SIZES):
            mean[:, k] = 3.0 * (2.0 * v[k].float() / (size - 1) - 1.0)
        logvar[:, :len(LAT_SIZES)] = -8.0 + 0.1 * torch.randn(N, len(LAT_SIZES), generator=gen, device="cuda")
    elif kind == "collapsed_7_of_10":
        mean[:, 3:] = 0.01 * torch.randn(N, D - 3, generator=gen, device="cuda")
        logvar[:, 3:] = 0.0
    return mean.contiguous(), logvar.contiguous()


def torch_mass(mean, logvar, rows, edges, out, chunk=16384):
    """out [D, n_bins * sum_sizes] fp64 in the layout of dvae_mass_joint."""
    nb, S = edges.numel() + 1, mean.shape[0] if rows is None else rows.numel()
    acc = [torch.zeros(size, D * nb, dtype=torch.float64, device="cuda") for size in LAT_SIZES]
    for s0 in range(0, S, chunk):
        r = torch.arange(s0, min(s0 + chunk, S), device="cuda") if rows is None else rows[s0:s0 + chunk]
        mu, den = mean[r].double(), torch.exp(0.5 * logvar[r].double()) * 1.4142135623730951
        t = (edges[None, None, :] - mu[:, :, None]) / den[:, :, None]
        up, dn = 0.5 * torch.erfc(t), 0.5 * torch.erfc(-t)
        q = torch.empty(r.numel(), D, nb, dtype=torch.float64, device="cuda")
        q[:, :, 0], q[:, :, nb - 1] = dn[:, :, 0], up[:, :, nb - 2]
        q[:, :, 1:nb - 1] = torch.where(t[:, :, :-1] >= 0, up[:, :, :-1] - up[:, :, 1:], dn[:, :, 1:] - dn[:, :, :-1])
        for a, v in zip(acc, factor_values(r, LAT_SIZES)):
            a.index_add_(0, v, q.view(r.numel(), D * nb))
    start = 0
    for a, size in zip(acc, LAT_SIZES):                               # [size, D, nb] -> [D, nb, size]
        out[:, start * nb:(start + size) * nb] = a.view(size, D, nb).permute(1, 2, 0).reshape(D, nb * size)
        start += size
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mass_time.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is nothing to time without it"
    M = _masslib.lib()
    N, K, sums = int(np.prod(LAT_SIZES)), len(LAT_SIZES), sum(LAT_SIZES)
    sizes = torch.tensor(LAT_SIZES, dtype=torch.int32, device="cuda")
    edges = torch.from_numpy(mass_edges(N_BINS)).cuda()
    lines = []
    for kind in TABLES:
        gen = torch.Generator(device="cuda").manual_seed(TABLES.index(kind) + 1)
        mean, logvar = make_table(kind, N, gen)
        for S in (N, 10000):
            rows = None if S == N else torch.randperm(N, generator=gen, device="cuda")[:S].contiguous()
            ws = torch.empty(M.dvae_mass_ws_doubles(N, D, K, S, N_BINS, sums), dtype=torch.float64, device="cuda")
            mass = torch.empty(D, N_BINS * sums, dtype=torch.float64, device="cuda")
            ref = torch.empty_like(mass)
            st = _stream()
            ours = median_ms(lambda: _masslib.call("dvae_mass_joint", mean.data_ptr(), logvar.data_ptr(),
                                                   None if rows is None else rows.data_ptr(), sizes.data_ptr(), edges.data_ptr(), N, D, K,
                                                   S, N_BINS, sums, ws.data_ptr(), mass.data_ptr(), st), args.reps)
            tor = median_ms(lambda: torch_mass(mean, logvar, rows, edges, ref), args.reps)
            diff = (mass - ref).abs().max().item()
            whole = []
            for rep in range(args.reps + 1):                          # the first is the warm-up
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                scores = interpretability_scores_from_table(mean, logvar, LAT_SIZES, n_bins=N_BINS, rows=rows)
                whole.append((time.perf_counter() - t0) * 1e3)
            whole = sorted(whole[1:])
            chunks, chunk_rows = _masslib.chunks(S)
            lines.append({
                "table": kind, "N": N, "D": D, "S": S, "n_bins": N_BINS, "lat_sizes": list(LAT_SIZES), "reps": args.reps,
                "workgroups": chunks * D * _masslib.column_groups(N_BINS, sums)[0], "rows_per_workgroup": chunk_rows,
                "erfc_evaluations": S * D * (-(-N_BINS // _masslib.WAVE_BINS)) * 64, "ws_MiB": round(ws.numel() * 8 / 2 ** 20, 1),
                "mass_joint_ms": round(ours[0], 3), "mass_joint_spread_ms": [round(ours[1], 3), round(ours[2], 3)],
                "torch_chunked_ms": round(tor[0], 3), "torch_spread_ms": [round(tor[1], 3), round(tor[2], 3)],
                "speedup_vs_torch": round(tor[0] / ours[0], 1), "max_abs_diff_vs_torch_fp64": diff,
                "max_abs_diff_over_rows_per_cell": diff / (S / max(LAT_SIZES)),
                "interpretability_scores_from_table_ms": round(whole[len(whole) // 2], 1),
                "interpretability_scores_from_table_spread_ms": [round(whole[0], 1), round(whole[-1], 1)],
                "rmig_norm": scores["rmig_norm"], "jemmig_norm": scores["jemmig_norm"], "mig_sup": scores["mig_sup"],
                "dcimig": scores["dcimig"]})
            print(json.dumps(lines[-1]), flush=True)
            del ws, mass, ref
        del mean, logvar
        torch.cuda.empty_cache()
    if args.bench:
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "200", "--warmup", "20"],
                             capture_output=True, text=True, cwd=ROOT)
        result = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
        lines.append({"bench_py": json.loads(result[-1]) if result else None, "bench_rc": out.returncode})
        print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
