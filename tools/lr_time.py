"""Cost of the linear-softmax probes fitted on the device (dvae_lr_fit / dvae_lr_predict, csrc/softmax_fit.hip) at the dSprites shape
(N = 737 280 rows, lat_sizes (3, 6, 40, 32, 32), D = 10; 10 000 rows to fit and 5 000 to test: five problems of 3 / 6 / 40 / 32 / 32
classes in one launch) on two tables -- Gaussian means; sharp, factor-aligned latents -- next to the host fit they stand in for:
explicitness_from_table and factor_scores_from_table with fit="host" and with fit="device", infoe_from_table, and (--sklearn)
scikit-learn's LogisticRegression(C=1.0) on the same rows on this machine's CPU.
--bench also runs `python bench.py` in a process of its own and records its result line: training does not load this library.

Device events around each launch; the candidates are interleaved within a round and the rounds repeated `--reps` times after a
warm-up round: the median and the spread over the rounds.  The whole *_from_table calls are timed by the host clock (they end in a
device->host copy), `--host-reps` rounds of those that run the host's L-BFGS.  One JSON line per table is printed and appended to
--out (profiles/lr_time.jsonl).  No speed-up is promised: what is measured is reported, the solver's step counts with it.

    python tools/lr_time.py [--reps 5] [--host-reps 1] [--sklearn] [--bench] [--out profiles/lr_time.jsonl]
"""
import argparse
import json
import os
import subprocess
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "disentangling-vae_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from disvae_amd import _lrlib, explicitness_from_table, infoe_from_table  # noqa: E402
from disvae_amd.engine import _stream  # noqa: E402
from disvae_amd.evaluate import factor_scores_from_table  # noqa: E402

LAT_SIZES, D, N_TRAIN, N_TEST, C = (3, 6, 40, 32, 32), 10, 10000, 5000, 1.0
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


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--sklearn", action="store_true")
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lr_time.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is nothing to time without it"
    L = _lrlib.lib()
    N, K, st = int(np.prod(LAT_SIZES)), len(LAT_SIZES), _stream()
    n, cls = list(LAT_SIZES), _lrlib.host_classes(LAT_SIZES)
    setups, candidates = {}, []
    for kind in TABLES:
        gen = torch.Generator(device="cuda").manual_seed(TABLES.index(kind) + 1)
        mean = make_table(kind, N, gen)
        rows = torch.randperm(N, generator=gen, device="cuda")[:N_TRAIN + N_TEST].contiguous()
        x = mean.index_select(0, rows)
        lab = torch.stack(factor_values(rows, LAT_SIZES)).to(torch.int32)          # 10 000 rows hold every value of every factor: ranks are values
        s = dict(mean=mean, rows=rows, xt=x[:N_TRAIN].contiguous(), xe=x[N_TRAIN:].contiguous(), lt=lab[:, :N_TRAIN].contiguous(),
                 le=lab[:, N_TRAIN:].contiguous(), ws=torch.empty(L.dvae_lr_ws_bytes(N_TRAIN, D, cls, K) // 8, dtype=torch.float64, device="cuda"),
                 coef=torch.empty(sum(_lrlib.coef_sizes(n, D)), dtype=torch.float64, device="cuda"),
                 report=torch.empty(K, 4, dtype=torch.float64, device="cuda"),
                 prob=torch.empty(N_TEST * sum(n), dtype=torch.float32, device="cuda"), loss=torch.empty(K, dtype=torch.float64, device="cuda"),
                 correct=torch.empty(K, dtype=torch.int32, device="cuda"), counted=torch.empty(K, dtype=torch.int32, device="cuda"))
        assert all(int(s["lt"][k].max()) == size - 1 and len(torch.unique(s["lt"][k])) == size for k, size in enumerate(LAT_SIZES))
        setups[kind] = s
        candidates += [
            (kind, "fit", lambda s=s: _lrlib.call("dvae_lr_fit", s["xt"].data_ptr(), None, None, s["lt"].data_ptr(), cls, N_TRAIN, D, K, C, 1e-8,
                                                  s["ws"].data_ptr(), s["coef"].data_ptr(), s["report"].data_ptr(), st)),
            (kind, "predict_test_with_prob", lambda s=s: _lrlib.call("dvae_lr_predict", s["xe"].data_ptr(), None, None, s["le"].data_ptr(), cls, N_TEST, D,
                                                                     K, s["coef"].data_ptr(), s["prob"].data_ptr(), s["loss"].data_ptr(),
                                                                     s["correct"].data_ptr(), s["counted"].data_ptr(), st)),
            (kind, "predict_test", lambda s=s: _lrlib.call("dvae_lr_predict", s["xe"].data_ptr(), None, None, s["le"].data_ptr(), cls, N_TEST, D, K,
                                                           s["coef"].data_ptr(), None, s["loss"].data_ptr(), s["correct"].data_ptr(),
                                                           s["counted"].data_ptr(), st)),
        ]
    times = {(kind, what): [] for kind, what, _fn in candidates}
    for rnd in range(args.reps + 1):                                  # the first round is the warm-up
        for kind, what, fn in candidates:                             # interleaved: every candidate once per round
            ms = timed(fn)
            if rnd:
                times[(kind, what)].append(ms)
    whole = {(kind, what): [] for kind in TABLES for what in ("explicitness_host", "explicitness_device", "infoe", "factor_scores_host",
                                                               "factor_scores_device")}
    scores = {}
    for rnd in range(args.reps + 1):                                  # the device fits: the first round is the warm-up; the tables interleaved
        for kind in TABLES:
            s = setups[kind]
            for what, fn in (("explicitness_device", lambda: explicitness_from_table(s["mean"], LAT_SIZES, rows=s["rows"], fit="device")),
                             ("infoe", lambda: infoe_from_table(s["mean"], LAT_SIZES, rows=s["rows"])),
                             ("factor_scores_device", lambda: factor_scores_from_table(s["mean"], LAT_SIZES, fit="device"))):
                ms, scores[(kind, what)] = wall(fn)
                if rnd:
                    whole[(kind, what)].append(ms)
    for rnd in range(args.host_reps):                                 # the host fits: seconds each, no warm-up
        for kind in TABLES:
            s = setups[kind]
            for what, fn in (("explicitness_host", lambda: explicitness_from_table(s["mean"], LAT_SIZES, rows=s["rows"])),
                             ("factor_scores_host", lambda: factor_scores_from_table(s["mean"], LAT_SIZES))):
                ms, scores[(kind, what)] = wall(fn)
                whole[(kind, what)].append(ms)
    sk_ms = {kind: [] for kind in TABLES}
    if args.sklearn:
        from sklearn.linear_model import LogisticRegression
        for kind in TABLES:
            s = setups[kind]
            X, y = s["xt"].cpu().numpy().astype(np.float64), s["lt"].cpu().numpy()
            t0 = time.perf_counter()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                for k in range(K):
                    LogisticRegression(C=C, tol=1e-8, max_iter=10000).fit(X, y[k])
            sk_ms[kind].append((time.perf_counter() - t0) * 1e3)
    lines = []
    for kind in TABLES:
        s = setups[kind]
        report = s["report"].cpu().numpy()
        line = {"table": kind, "N": N, "D": D, "lat_sizes": list(LAT_SIZES), "n_train": N_TRAIN, "n_test": N_TEST, "C": C, "reps": args.reps,
                "host_reps": args.host_reps, "tolerance_grad": 1e-8, "ws_bytes": int(s["ws"].numel() * 8)}
        for what in ("fit", "predict_test_with_prob", "predict_test"):
            line["%s_ms" % what], line["%s_spread_ms" % what] = stats(times[(kind, what)])
        for what in ("explicitness_host", "explicitness_device", "infoe", "factor_scores_host", "factor_scores_device"):
            if whole[(kind, what)]:
                line["%s_from_table_ms" % what], line["%s_spread_ms" % what] = stats(whole[(kind, what)])
        line.update(newton_steps=[int(v) for v in report[:, 2]], function_evaluations=[int(v) for v in report[:, 3]],
                    max_abs_gradient=float(report[:, 1].max()), infoe_train=scores[(kind, "infoe")]["infoe_train"],
                    infoe_test=scores[(kind, "infoe")]["infoe_test"],
                    explicitness_test_device=scores[(kind, "explicitness_device")]["explicitness_test"],
                    beta_vae_eval_device=scores[(kind, "factor_scores_device")]["beta_vae_eval"])
        if args.host_reps:
            line.update(explicitness_test_host=scores[(kind, "explicitness_host")]["explicitness_test"],
                        beta_vae_eval_host=scores[(kind, "factor_scores_host")]["beta_vae_eval"])
        if args.sklearn:
            line["sklearn_5_fits_ms"] = round(sk_ms[kind][0], 1)
            line["cpu_threads_env"] = os.environ.get("OMP_NUM_THREADS")
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
