"""Cost of the binning-free mutual-information scores behind Evaluator.compute_knn_information_scores (dvae_knn_sort / dvae_knn_mi,
csrc/knn_mi.hip) at the dSprites shape (N = 737 280 rows, lat_sizes (3, 6, 40, 32, 32), D = 10; 10 000 drawn rows, n_neighbors = 3:
50 (latent, factor) pairs) on two tables -- Gaussian means; sharp, factor-aligned latents -- next to what computes the same
without it: a torch restatement on the same GPU (sort, per-class masks, searchsorted; --torch) and the 50 calls of scikit-learn's
_compute_mi_cd on this machine's CPU (--sklearn).
--bench also runs `python bench.py` in a process of its own and records its result line: training does not load this library.

Device events around each launch; the candidates (two launches x two tables) are interleaved within a round and the rounds repeated
`--reps` times after a warm-up round: the median and the spread over the rounds.  The whole knn_information_scores_from_table call
is timed by the host clock (it ends in the device->host copy), and so are the torch restatement (it ends in a synchronisation) and
scikit-learn's loop, `--sklearn-reps` rounds without a warm-up.  One JSON line per table is printed and appended to --out
(profiles/knn_time.jsonl).  No speed-up is promised: what is measured is reported.

    python tools/knn_time.py [--reps 7] [--torch] [--sklearn] [--sklearn-reps 3] [--bench] [--out profiles/knn_time.jsonl]
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

from disvae_amd import _knnlib, digamma_integers, knn_information_scores_from_table  # noqa: E402
from disvae_amd.engine import _stream  # noqa: E402

LAT_SIZES, D, S, KN = (3, 6, 40, 32, 32), 10, 10000, 3
TABLES = ("gaussian", "sharp_aligned")


def factor_values(rows, lat_sizes):
    out, stride = [], 1
    for size in reversed(lat_sizes):
        out.append((rows // stride) % size)
        stride *= size
    return out[::-1]


def make_table(kind, N, gen):
    mean = torch.randn(N, D, generator=gen, device="cuda")
    if kind == "sharp_aligned":                                       # latent k holds factor k, the other five are noise
        v = factor_values(torch.arange(N, device="cuda"), LAT_SIZES)
        for k, size in enumerate(LAT_SIZES):
            mean[:, k] = 3.0 * (2.0 * v[k].float() / (size - 1) - 1.0) + 0.02 * torch.randn(N, generator=gen, device="cuda")
    return mean.contiguous()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(times):
    times = sorted(times)
    return round(times[len(times) // 2], 3), [round(times[0], 3), round(times[-1], 3)]


def torch_restatement(mean, rows, psi):
    """The estimator with torch's own kernels: a sort per column; per (column, factor) a mask, a sort and a window per class for
    the radius, two searchsorted per row for the count (x -+ r: rounded, where the library compares exact differences)."""
    x_all = mean.index_select(0, rows).double()
    values = factor_values(rows, LAT_SIZES)
    raw = torch.zeros(D, len(LAT_SIZES), dtype=torch.float64, device="cuda")
    inf = torch.full((KN,), float("inf"), dtype=torch.float64, device="cuda")
    for d in range(D):
        x = x_all[:, d].contiguous()
        for k, size in enumerate(LAT_SIZES):
            v = values[k]
            c = torch.bincount(v, minlength=size)[v]
            keep = c >= 2
            radius = torch.zeros_like(x)
            k_i = torch.clamp(c - 1, max=KN)
            for value in range(size):
                members = torch.nonzero(v == value).view(-1)
                cnt = int(members.numel())
                if cnt < 2:
                    continue
                a, order = torch.sort(x[members])
                kk = min(KN, cnt - 1)
                window = torch.cat([inf[:kk], a, inf[:kk]]).unfold(0, 2 * kk + 1, 1)
                radius[members[order]] = (window - a[:, None]).abs().sort(dim=1).values[:, kk]
            xs = torch.sort(x[keep]).values
            xi, ri = x[keep], radius[keep]
            strict = torch.searchsorted(xs, xi + ri, right=False) - torch.searchsorted(xs, xi - ri, right=True)
            equal = torch.searchsorted(xs, xi, right=True) - torch.searchsorted(xs, xi, right=False)
            m = torch.where(ri > 0, strict, equal)
            n = int(keep.sum())
            raw[d, k] = psi[n] + psi[k_i[keep]].mean() - psi[c[keep]].mean() - psi[m].mean()
    torch.cuda.synchronize()
    return raw.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--torch", action="store_true")
    ap.add_argument("--sklearn", action="store_true")
    ap.add_argument("--sklearn-reps", type=int, default=3)
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_time.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is nothing to time without it"
    h = _knnlib.lib()
    N, K, st = int(np.prod(LAT_SIZES)), len(LAT_SIZES), _stream()
    sizes = _knnlib.host_sizes(LAT_SIZES)
    psi = torch.from_numpy(digamma_integers(S)).cuda()
    setups, candidates = {}, []
    for kind in TABLES:
        gen = torch.Generator(device="cuda").manual_seed(TABLES.index(kind) + 1)
        mean = make_table(kind, N, gen)
        rows = torch.randperm(N, generator=gen, device="cuda")[:S].contiguous()
        ws = torch.empty(h.dvae_knn_ws_bytes(N, D, S), dtype=torch.uint8, device="cuda")
        sums = torch.empty(D, K, 4, dtype=torch.float64, device="cuda")
        counts = torch.empty(K, sum(LAT_SIZES), dtype=torch.int32, device="cuda")
        setups[kind] = s = dict(mean=mean, rows=rows, ws=ws, sums=sums, counts=counts)
        candidates += [
            (kind, "sort", lambda s=s: _knnlib.call("dvae_knn_sort", s["mean"].data_ptr(), s["rows"].data_ptr(), N, D, S, s["ws"].data_ptr(), st)),
            (kind, "mi", lambda s=s: _knnlib.call("dvae_knn_mi", s["rows"].data_ptr(), sizes, N, D, K, S, KN, psi.data_ptr(), s["ws"].data_ptr(),
                                                  s["sums"].data_ptr(), s["counts"].data_ptr(), None, None, st)),
        ]
    times = {(kind, what): [] for kind, what, _fn in candidates}
    for rnd in range(args.reps + 1):                                  # the first round is the warm-up
        for kind, what, fn in candidates:                             # interleaved: every candidate once per round
            ms = timed(fn)
            if rnd:
                times[(kind, what)].append(ms)
    whole, scores = {kind: [] for kind in TABLES}, {}
    for rnd in range(args.reps + 1):                                  # the first round is the warm-up; the tables interleaved
        for kind in TABLES:
            s = setups[kind]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            scores[kind] = knn_information_scores_from_table(s["mean"], LAT_SIZES, n_neighbors=KN, rows=s["rows"])
            if rnd:
                whole[kind].append((time.perf_counter() - t0) * 1e3)
    torch_ms, torch_raw = {kind: [] for kind in TABLES}, {}
    if args.torch:
        for rnd in range(3):                                          # the first round is the warm-up
            for kind in TABLES:
                s = setups[kind]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                torch_raw[kind] = torch_restatement(s["mean"], s["rows"], psi)
                if rnd:
                    torch_ms[kind].append((time.perf_counter() - t0) * 1e3)
    sk_ms, sk_mi = {kind: [] for kind in TABLES}, {}
    if args.sklearn:
        from sklearn.feature_selection._mutual_info import _compute_mi_cd
        host = {}
        for kind in TABLES:
            s = setups[kind]
            host[kind] = (s["mean"].index_select(0, s["rows"]).cpu().numpy().astype(np.float64),
                          [v.cpu().numpy() for v in factor_values(s["rows"], LAT_SIZES)])
        for rnd in range(args.sklearn_reps):
            for kind in TABLES:
                X, values = host[kind]
                matrix = np.zeros((D, K))
                t0 = time.perf_counter()
                for i in range(D):
                    for j in range(K):
                        matrix[i, j] = _compute_mi_cd(X[:, i], values[j], KN)
                sk_ms[kind].append((time.perf_counter() - t0) * 1e3)
                sk_mi[kind] = matrix
    lines = []
    for kind in TABLES:
        got = scores[kind]
        sort_lds, mi_lds = _knnlib.lds_bytes(S)
        line = {"table": kind, "N": N, "D": D, "lat_sizes": list(LAT_SIZES), "n_samples": S, "n_neighbors": KN, "reps": args.reps,
                "pairs": D * K, "sort_lds_bytes_per_workgroup": sort_lds, "mi_lds_bytes_per_workgroup": mi_lds}
        for what in ("sort", "mi"):
            line["%s_ms" % what], line["%s_spread_ms" % what] = stats(times[(kind, what)])
        line["knn_information_scores_from_table_ms"], line["knn_information_scores_from_table_spread_ms"] = stats(whole[kind])
        line.update({key: got[key] for key in ("mig", "mig_sup", "dcimig", "modularity", "infom", "infoc", "n_active")})
        if args.torch:
            line["torch_restatement_ms"], line["torch_restatement_spread_ms"] = stats(torch_ms[kind])
            line["torch_restatement_raw_max_abs_diff"] = float(np.abs(torch_raw[kind] - got["raw"]).max())
        if args.sklearn:
            line["sklearn_50_compute_mi_cd_ms"], line["sklearn_spread_ms"] = stats(sk_ms[kind])
            line.update(sklearn_reps=args.sklearn_reps, sklearn_mi_max_abs_diff=float(np.abs(sk_mi[kind] - got["mutual_information"]).max()),
                        cpu_threads_env=os.environ.get("OMP_NUM_THREADS"))
        lines.append(line)
        print(json.dumps(line), flush=True)
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
