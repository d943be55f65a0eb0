"""Cost of the ranking kernels (libdvae_udr_hip.so, csrc/latent_ranks.hip) and of the whole udr_from_tables at the dSprites shape
(N = 737 280, D = 10) -- all rows, and 10 000 drawn rows -- next to the torch code a user would write without them on the same
GPU: per column one sort plus searchsorted left and right for the tie-averaged ranks, batched on the device, no copy in between.

Three tables: "gauss" (independent Gaussian columns), "collapsed" (7 of the 10 columns exactly constant, as the unused dimensions
of a trained VAE: every key of such a column is one run) and "ties" (values rounded to 1 / 64: runs of thousands).  Device events
around each call, `--reps` repeats after a warm-up, the median and the spread; inputs from a seed.  The ranks of both versions
are compared for EQUALITY before timing.  Also the KL pass, and the whole udr_from_tables for M = 5 models (wall clock, both
correlations).  Prints one JSON line per measurement and writes them to --out.

    python tools/udr_time.py [--reps 20] [--out profiles/udr_time.jsonl]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "disentangling-vae_amd")]

import torch  # noqa: E402

from disvae_amd import _udrlib  # noqa: E402
from disvae_amd.engine import _stream  # noqa: E402
from disvae_amd.evaluate import udr_from_tables  # noqa: E402

N, D, DRAWN, MODELS = 737280, 10, 10000, 5


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


def torch_ranks(picked):
    """per column: sort, then searchsorted left and right -> #{smaller} + (#{equal} + 1) / 2"""
    out = torch.empty_like(picked)
    for d in range(picked.shape[1]):
        col = (picked[:, d] + 0.0).contiguous()
        srt = torch.sort(col).values
        lo, hi = torch.searchsorted(srt, col, right=False), torch.searchsorted(srt, col, right=True)
        out[:, d] = lo.float() + (hi - lo + 1).float() * 0.5
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "udr_time.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is nothing to time without it"
    lines = []

    def emit(what, t, **more):
        lines.append(json.dumps(dict({"what": what, "N": N, "D": D, "reps": args.reps, "median_ms": t[0], "spread_ms": t[1]}, **more)))
        print(lines[-1], flush=True)

    gen = torch.Generator(device="cuda").manual_seed(1)
    gauss = torch.randn(N, D, generator=gen, device="cuda")
    collapsed = gauss.clone()
    collapsed[:, 3:] = torch.linspace(-1, 1, 7, device="cuda")
    tables = {"gauss": gauss.contiguous(), "collapsed": collapsed.contiguous(), "ties": (torch.round(gauss * 64) / 64).contiguous()}
    logvar = (-6 + 0.3 * torch.randn(N, D, generator=gen, device="cuda")).contiguous()
    drawn = torch.randperm(N, generator=gen, device="cuda")[:DRAWN].contiguous()
    h = _udrlib.lib()
    ws = torch.empty(max(h.dvae_udr_ranks_ws_floats(N, D, N), h.dvae_udr_kl_dims_ws_floats(N, D, N)), device="cuda")
    kl = torch.empty(D, dtype=torch.float64, device="cuda")
    st = _stream()
    for name, table in tables.items():
        for rows, S, sel in ((None, N, "all rows"), (drawn, DRAWN, "%d drawn rows" % DRAWN)):
            rp = None if rows is None else rows.data_ptr()
            picked = table if rows is None else table[rows]
            ranks = torch.empty(S, D, device="cuda")

            def native():
                _udrlib.call("dvae_udr_ranks", table.data_ptr(), rp, N, D, S, ws.data_ptr(), ranks.data_ptr(), st)
            native()
            same = bool(torch.equal(torch_ranks(picked), ranks))
            assert same, "the kernel's ranks differ from torch's"
            more = dict(table=name, rows=sel, S=S)
            emit("dvae_udr_ranks", median_ms(native, args.reps), table_bytes=N * D * 4, ranks_equal_torch=same, **more)
            emit("torch: per column sort + searchsorted left and right", median_ms(lambda: torch_ranks(picked), args.reps), **more)
            if name == "gauss":
                def kl_dims():
                    _udrlib.call("dvae_udr_kl_dims", table.data_ptr(), logvar.data_ptr(), rp, N, D, S, ws.data_ptr(), kl.data_ptr(), st)
                kl_dims()
                mu64, lv64 = picked.double(), (logvar if rows is None else logvar[rows]).double()
                ref = (0.5 * (mu64 * mu64 + lv64.exp() - lv64 - 1)).mean(0)
                err = float(((kl - ref).abs() / ref).max())
                assert err < 1e-9, err
                emit("dvae_udr_kl_dims", median_ms(kl_dims, args.reps), kl_vs_torch_rel=err, **more)
                emit("torch: the KL per dimension of the fp64 tables",
                     median_ms(lambda: (0.5 * (picked.double() ** 2 + (logvar if rows is None else logvar[rows]).double().exp()
                                               - (logvar if rows is None else logvar[rows]).double() - 1)).mean(0), args.reps), **more)
    # the whole call for a sweep of five models: signed, permuted copies of one table plus noise
    means = []
    for m in range(MODELS):
        perm = torch.randperm(D, generator=gen, device="cuda")
        means.append((gauss[:, perm] * (1 if m % 2 else -1) + 0.05 * torch.randn(N, D, generator=gen, device="cuda")).contiguous())
    logvars = [logvar] * MODELS
    for correlation in ("spearman", "lasso"):
        for rows, S, sel in ((None, N, "all rows"), (drawn, DRAWN, "%d drawn rows" % DRAWN)):
            def whole():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                udr_from_tables(means, logvars, correlation=correlation, rows=rows)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3
            whole()
            w = sorted(whole() for _ in range(5))
            emit("udr_from_tables, M = 5 (%s; every launch, the copies, the host's fp64), wall clock" % correlation,
                 (round(w[2], 2), [round(w[0], 2), round(w[4], 2)]), rows=sel, S=S, models=MODELS)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
