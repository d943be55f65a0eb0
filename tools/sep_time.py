"""Cost of the leave-one-out log-densities behind Evaluator.compute_separability_scores (dvae_sep_loo_logq, csrc/latent_loo.hip)
at dSprites size and at S = N = 10 000 drawn rows, next to what computes the same without it:
  (a) the shipped dvae_eval_joint_logq once, at the same shape (one of the D + 1 results);
  (b) D calls of dvae_eval_joint_logq on the D column-deleted tables, their preparation (the copies of mean, logvar and z without
      the column) included, plus the one on the full table: the same D + 1 results with shipped code;
  (c) the torch code a user would write -- chunked [S_chunk, N, D] log-densities, D + 1 sums over the kept columns and their
      logsumexp, the temporary sized to 2 GiB -- on the same GPU;
  (d) the whole compute_separability_scores call on a model whose encoder looks the table up (host clock, ends in the
      device->host copy).

Device events around each call, `--reps` repeats after a warm-up, the median and the spread; inputs from a seed.  The torch
baseline is timed on its first `--torch-samples` samples and scaled to S (its chunks are independent and equal): marked
"extrapolated".  Prints one JSON line per shape.

    python tools/sep_time.py [--reps 5] [--torch-samples 1000]
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "disentangling-vae_amd")]

import torch  # noqa: E402

from disvae_amd import _evallib, _seplib, Evaluator  # noqa: E402
from disvae_amd.engine import _stream  # noqa: E402

SHAPES = [(737280, 10, 10000), (10000, 10, 10000)]
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


def torch_loo_logq(z, mean, logvar, out, budget_bytes=2 << 30):
    N, D = mean.shape
    step = max(1, budget_bytes // (N * D * 4))
    c, iv = -0.5 * (LOG2PI + logvar), torch.exp(-logvar)
    keep = [[d for d in range(D) if d != i] for i in range(D)] + [list(range(D))]
    for s0 in range(0, z.shape[0], step):
        ld = c[None] - 0.5 * (z[s0:s0 + step, None, :] - mean[None]) ** 2 * iv[None]
        for i, cols in enumerate(keep):
            out[i, s0:s0 + step] = torch.logsumexp(ld[:, :, cols].sum(2), 1) - math.log(N)
    return out


class TableModel(torch.nn.Module):
    """A model whose encoder looks q(z|x) up in a table: image x is its row number."""

    def __init__(self, mean, logvar):
        super().__init__()
        self.latent_dim = mean.shape[1]
        self.mean, self.logvar = mean, logvar

    def encoder(self, x):
        idx = x.view(-1).long()
        return self.mean[idx], self.logvar[idx]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torch-samples", type=int, default=1000)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is nothing to time without it"
    E, P = _evallib.lib(), _seplib.lib()
    for N, D, S in SHAPES:
        gen = torch.Generator(device="cuda").manual_seed(N + D + S)
        centers = 2.0 * torch.randn(8, D, generator=gen, device="cuda")
        mean = 0.3 * torch.randn(N, D, generator=gen, device="cuda") + centers[torch.arange(N, device="cuda") % 8]
        logvar = -2.0 + 2.5 * torch.rand(N, D, generator=gen, device="cuda")
        rows = torch.randperm(N, generator=gen, device="cuda")[:S]
        z = (mean[rows] + torch.exp(0.5 * logvar[rows]) * torch.randn(S, D, generator=gen, device="cuda")).contiguous()
        ws = torch.empty(max(E.dvae_eval_joint_logq_ws_floats(N, D, S), P.dvae_sep_loo_logq_ws_floats(N, D, S)), device="cuda")
        logq, H64 = torch.empty(D + 1, S, device="cuda"), torch.empty(D + 1, dtype=torch.float64, device="cuda")
        shipped, H = torch.empty(D + 1, S, device="cuda"), torch.empty(1, device="cuda")
        st = _stream()

        def joint(zz, mm, ll, out):
            _evallib.call("dvae_eval_joint_logq", zz.data_ptr(), mm.data_ptr(), ll.data_ptr(), N, mm.shape[1], S, ws.data_ptr(),
                          out.data_ptr(), H.data_ptr(), st)

        def separate_passes():
            for i in range(D):
                cols = torch.tensor([d for d in range(D) if d != i], device="cuda")
                joint(z.index_select(1, cols), mean.index_select(1, cols), logvar.index_select(1, cols), shipped[i])
            joint(z, mean, logvar, shipped[D])

        fused = median_ms(lambda: _seplib.call("dvae_sep_loo_logq", z.data_ptr(), mean.data_ptr(), logvar.data_ptr(), N, D, S,
                                               ws.data_ptr(), logq.data_ptr(), H64.data_ptr(), st), args.reps)
        fused_logq = logq.clone()
        one = median_ms(lambda: joint(z, mean, logvar, shipped[D]), args.reps)
        sep = median_ms(separate_passes, args.reps)
        diff_shipped = (fused_logq - shipped).abs().max().item()
        St = min(S, args.torch_samples)
        ref = torch.empty(D + 1, St, device="cuda")
        tor = median_ms(lambda: torch_loo_logq(z[:St], mean, logvar, ref), args.reps)
        scale = S / St
        diff_torch = (fused_logq[:, :St] - ref).abs().max().item()

        model = TableModel(mean, logvar)
        ev = Evaluator(model, None, device=torch.device("cuda"), is_progress_bar=False)
        loader = [(torch.arange(lo, min(lo + 65536, N), dtype=torch.float32, device="cuda").view(-1, 1), None)
                  for lo in range(0, N, 65536)]
        whole = []
        for rep in range(args.reps + 1):                              # the first is the warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            scores = ev.compute_separability_scores(loader, n_samples=S, seed=rep)
            whole.append((time.perf_counter() - t0) * 1e3)
        whole = sorted(whole[1:])
        print(json.dumps({
            "N": N, "D": D, "S": S, "reps": args.reps,
            "loo_logq_ms": round(fused[0], 3), "loo_logq_spread_ms": [round(fused[1], 3), round(fused[2], 3)],
            "joint_logq_ms": round(one[0], 3), "joint_logq_spread_ms": [round(one[1], 3), round(one[2], 3)],
            "separate_joint_passes_ms": round(sep[0], 3), "separate_joint_passes_spread_ms": [round(sep[1], 3), round(sep[2], 3)],
            "loo_over_joint": round(fused[0] / one[0], 2), "separate_over_loo": round(sep[0] / fused[0], 2),
            "torch_chunked_ms": round(tor[0] * scale, 1), "torch_extrapolated": St < S, "torch_samples_timed": St,
            "torch_spread_ms": [round(tor[1] * scale, 1), round(tor[2] * scale, 1)],
            "speedup_vs_torch": round(tor[0] * scale / fused[0], 1),
            "compute_separability_scores_ms": round(whole[len(whole) // 2], 1),
            "compute_separability_scores_spread_ms": [round(whole[0], 1), round(whole[-1], 1)],
            "max_abs_diff_vs_separate_passes": diff_shipped, "max_abs_diff_vs_torch_fp32": diff_torch,
            "wsepin": scores["wsepin"], "H_z": H64[D].item()}), flush=True)
        del ws, mean, logvar, z, ref, logq, shipped, model, ev, loader
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
