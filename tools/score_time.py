"""Cost of the FactorVAE / beta-VAE score kernels (libdvae_score_hip.so, csrc/factor_scores.hip) and of the whole
factor_scores_from_table at dSprites size (N = 737 280, D = 10, 10 000 + 5 000 groups of 64, 10 000 variance rows), next to the
torch code a user would write without them on the same GPU: (a) one index_select + var + argmin per group in a Python loop,
(b) the same batched as one [V, L, D] gather.

Device events around each call, `--reps` repeats after a warm-up, the median; inputs from a seed.  The Python loop is timed on
its first `--loop-groups` groups and scaled to V (its iterations are independent and equal): marked "extrapolated".  Prints one
JSON line per measurement.

    python tools/score_time.py [--reps 5] [--loop-groups 2000]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "disentangling-vae_amd")]

import torch  # noqa: E402

from disvae_amd import _scorelib  # noqa: E402
from disvae_amd.engine import _stream  # noqa: E402
from disvae_amd.evaluate import draw_fixed_factor_rows, factor_scores_from_table  # noqa: E402

LAT = (3, 6, 40, 32, 32)
N, D, V, L, NVAR = 737280, 10, 15000, 64, 10000


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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-groups", type=int, default=2000)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is nothing to time without it"
    gen = torch.Generator(device="cuda").manual_seed(1)
    table = torch.randn(N, D, generator=gen, device="cuda").contiguous()
    factor, rows = draw_fixed_factor_rows(LAT, V, L, gen, device="cuda")
    _, rows_a, rows_b = draw_fixed_factor_rows(LAT, V, L, gen, device="cuda", paired=True)
    var_rows = torch.randperm(N, generator=gen, device="cuda")[:NVAR].contiguous()
    inv = (1.0 / table.index_select(0, var_rows).var(0)).contiguous()
    active = torch.ones(D, dtype=torch.int32, device="cuda")
    K = len(LAT)
    stat, out1 = torch.empty(V, D, device="cuda"), torch.empty(1, D, device="cuda")
    argmin, votes = torch.empty(V, dtype=torch.int32, device="cuda"), torch.empty(K, D, dtype=torch.int32, device="cuda")
    st = _stream()

    def emit(what, t, **more):
        print(json.dumps(dict({"what": what, "N": N, "D": D, "reps": args.reps, "median_ms": t[0], "spread_ms": t[1]}, **more)),
              flush=True)

    emit("dvae_score_group_var V=15000 L=64 (a group per wave)", median_ms(lambda: _scorelib.call(
        "dvae_score_group_var", table.data_ptr(), rows.data_ptr(), N, D, V, L, inv.data_ptr(), None, stat.data_ptr(), st), args.reps),
        gathered_bytes=V * L * D * 4)
    emit("dvae_score_group_var V=1 L=10000 (a group per workgroup)", median_ms(lambda: _scorelib.call(
        "dvae_score_group_var", table.data_ptr(), var_rows.data_ptr(), N, D, 1, NVAR, None, None, out1.data_ptr(), st), args.reps))
    emit("dvae_score_pair_absdiff V=15000 L=64", median_ms(lambda: _scorelib.call(
        "dvae_score_pair_absdiff", table.data_ptr(), rows_a.data_ptr(), rows_b.data_ptr(), N, D, V, L, stat.data_ptr(), st), args.reps),
        gathered_bytes=2 * V * L * D * 4)
    _scorelib.call("dvae_score_group_var", table.data_ptr(), rows.data_ptr(), N, D, V, L, inv.data_ptr(), None, stat.data_ptr(), st)
    emit("dvae_score_vote V=15000 K=5", median_ms(lambda: _scorelib.call(
        "dvae_score_vote", stat.data_ptr(), factor.data_ptr(), active.data_ptr(), V, D, K, argmin.data_ptr(), votes.data_ptr(), st),
        args.reps))
    kernel_argmin = argmin.clone()

    # the torch restatements of the FactorVAE statistic + vote
    def batched():
        s = table[rows].var(1) * inv                                   # [V, L, D] gather
        a = s.argmin(1)
        return torch.zeros(K * D, dtype=torch.int64, device="cuda").index_add_(0, factor.long() * D + a, torch.ones_like(a)), a
    emit("torch batched [V, L, D] gather + var + argmin + vote, V=15000", median_ms(batched, args.reps))
    same = (batched()[1].int() == kernel_argmin).float().mean().item()
    G = min(V, args.loop_groups)

    def loop():
        a = torch.empty(G, dtype=torch.int64, device="cuda")
        for v in range(G):
            a[v] = (table.index_select(0, rows[v]).var(0) * inv).argmin()
        return a
    t = median_ms(loop, max(1, args.reps // 2))
    emit("torch Python loop: index_select + var + argmin per group, V=15000", (round(t[0] * V / G, 1), [round(x * V / G, 1) for x in t[1]]),
         extrapolated=G < V, groups_timed=G, argmin_agreement_batched_vs_kernel=same)

    # the whole of factor_scores_from_table (draws, kernels, copies, the classifier fit on the host), wall clock
    def whole():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        factor_scores_from_table(table, LAT)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    whole()
    w = sorted(whole() for _ in range(3))
    emit("factor_scores_from_table (10000 + 5000 groups of 64, 10000 variance rows), wall clock incl. host classifier",
         (round(w[1], 1), [round(w[0], 1), round(w[2], 1)]))


if __name__ == "__main__":
    main()
