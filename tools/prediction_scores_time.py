"""Cost of the prediction-based scores -- downstream_task_from_table, fairness_from_table, explicitness_from_table -- at the dSprites
shape: a [737 280, 10] table, factors with 3 / 6 / 40 / 32 / 32 values, the defaults of disentanglement_lib (training sets of 10 /
100 / 1000 / 10 000 rows, 5 000 test rows, 100 stages; 10 000 training rows and 100 base rows per value; 10 000 + 5 000 rows),
next to the only alternative for the boosted trees without the device: scikit-learn's GradientBoostingClassifier().fit on the same
rows on this machine's CPU.

The table is synthetic, as in tools/dci_time.py: latent k follows factor k (noise of a third of a step), the other five latents are
noise.  Each call is timed on the wall clock between device synchronisations, `--reps` repeats after a warm-up, the median and the
spread.  For the downstream task the share of the fits is measured too: device events around every fit of a call (sort of the
columns excluded, labels and buffers included), summed, over the wall time of that call.  Explicitness is mostly the host's
L-BFGS fit of the logistic regression; its share is reported from a wall-clock timer around fit_logistic_regression.
scikit-learn (--sklearn): every factor at the two smallest training sets in full; the two larger ones are EXTRAPOLATED linearly in the
number of rows from the 100-row fit and marked so.  Prints one JSON line per measurement and writes them to --out.

    python tools/prediction_scores_time.py [--reps 3] [--sklearn] [--out profiles/prediction_scores_time.jsonl]
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

from disvae_amd import evaluate as E  # noqa: E402

LAT_SIZES, D, STAGES = (3, 6, 40, 32, 32), 10, 100
N_TRAIN, N_TEST, PER_VALUE = (10, 100, 1000, 10000), 5000, 100


def wall_ms(fn, reps):
    fn()                                                              # warm-up: code objects, allocator
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = fn()
        torch.cuda.synchronize()
        times.append(1000 * (time.perf_counter() - t0))
    times.sort()
    return round(times[len(times) // 2], 2), [round(times[0], 2), round(times[-1], 2)], got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sklearn", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prediction_scores_time.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is nothing to time without it"
    lines = []

    def emit(what, **more):
        lines.append(json.dumps(dict({"what": what, "D": D, "lat_sizes": list(LAT_SIZES)}, **more)))
        print(lines[-1], flush=True)

    n = int(np.prod(LAT_SIZES))
    gen = torch.Generator(device="cuda").manual_seed(1)
    idx = torch.arange(n, device="cuda")
    mean = torch.randn(n, D, generator=gen, device="cuda")
    strides = [int(np.prod(LAT_SIZES[k + 1:])) for k in range(len(LAT_SIZES))]
    for k, size in enumerate(LAT_SIZES):
        mean[:, k] = ((idx // strides[k]) % size).float() + mean[:, k] / 3
    mean = mean.contiguous()
    rows = [torch.randperm(n, generator=gen, device="cuda")[:size + N_TEST].contiguous() for size in N_TRAIN]

    # ---- downstream task, and the share of its fits
    fit_events = []
    plain = E._BoostedFactor

    class Timed(plain):
        def __init__(self, *a):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            plain.__init__(self, *a)
            e1.record()
            fit_events.append((e0, e1))

    def downstream():
        return E.downstream_task_from_table(mean, LAT_SIZES, n_train=N_TRAIN, n_test=N_TEST, rows=rows, n_stages=STAGES)
    E._BoostedFactor = Timed
    try:
        shares = []
        downstream()
        for _ in range(args.reps):
            del fit_events[:]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            downstream()
            torch.cuda.synchronize()
            whole = 1000 * (time.perf_counter() - t0)
            fits = sum(e0.elapsed_time(e1) for e0, e1 in fit_events)
            shares.append((whole, fits))
    finally:
        E._BoostedFactor = plain
    shares.sort()
    whole, fits = shares[len(shares) // 2]
    median, spread, got = wall_ms(downstream, args.reps)
    emit("downstream_task_from_table", n_train=list(N_TRAIN), n_test=N_TEST, stages=STAGES, reps=args.reps, median_ms=median,
         spread_ms=spread, fits=len(N_TRAIN) * len(LAT_SIZES), fits_ms=round(fits, 2), timed_call_ms=round(whole, 2),
         fit_share=round(fits / whole, 3),
         **{key: round(got[key], 4) for key in got if key.endswith("mean_test_accuracy") or key.endswith("efficiency")})

    # ---- fairness
    def fairness():
        return E.fairness_from_table(mean, LAT_SIZES, n_train=N_TRAIN[-1], n_test_per_value=PER_VALUE, seed=0, n_stages=STAGES)
    median, spread, got = wall_ms(fairness, args.reps)
    K = len(LAT_SIZES)
    emit("fairness_from_table", n_train=N_TRAIN[-1], n_test_per_value=PER_VALUE, stages=STAGES, reps=args.reps, median_ms=median,
         spread_ms=spread, fits=K, pairs=K * (K - 1), rows_predicted=sum(LAT_SIZES) * (K - 1) * PER_VALUE,
         mean_unfairness=round(got["mean_unfairness"], 4), max_unfairness=round(got["max_unfairness"], 4))

    # ---- explicitness (the fit of the logistic regression is the host's)
    host = [0.0]
    fit_lr = E.fit_logistic_regression

    def timed_lr(*a, **kw):
        t0 = time.perf_counter()
        out = fit_lr(*a, **kw)
        host[0] += 1000 * (time.perf_counter() - t0)
        return out

    def explicitness():
        host[0] = 0.0
        return E.explicitness_from_table(mean, LAT_SIZES, n_train=N_TRAIN[-1], n_test=N_TEST, rows=rows[-1])
    E.fit_logistic_regression = timed_lr
    try:
        median, spread, got = wall_ms(explicitness, args.reps)
    finally:
        E.fit_logistic_regression = fit_lr
    emit("explicitness_from_table", n_train=N_TRAIN[-1], n_test=N_TEST, reps=args.reps, median_ms=median, spread_ms=spread,
         host_fit_ms_last_rep=round(host[0], 2), host_threads=torch.get_num_threads(),
         explicitness_train=round(got["explicitness_train"], 4), explicitness_test=round(got["explicitness_test"], 4))

    if args.sklearn:
        from sklearn.ensemble import GradientBoostingClassifier
        for k, C in enumerate(LAT_SIZES):
            seconds = {}
            for size, rows_n in zip(N_TRAIN[:2], rows[:2]):
                train = rows_n[:size]
                X, y = mean.index_select(0, train).cpu().numpy(), ((train // strides[k]) % C).cpu().numpy()
                if len(np.unique(y)) < 2:                                # scikit-learn refuses one class
                    seconds[size] = None
                    continue
                t0 = time.perf_counter()
                GradientBoostingClassifier(n_estimators=STAGES, random_state=0).fit(X, y)
                seconds[size] = time.perf_counter() - t0
            base = seconds[N_TRAIN[1]]
            emit("sklearn GradientBoostingClassifier.fit", factor=k, classes=C, stages=STAGES,
                 seconds_timed={str(s): (None if v is None else round(v, 3)) for s, v in seconds.items()},
                 seconds_extrapolated={str(s): round(base * s / N_TRAIN[1], 1) for s in N_TRAIN[2:]},
                 extrapolation="linear in the number of rows from the %d-row fit" % N_TRAIN[1],
                 cpu_threads_env=os.environ.get("OMP_NUM_THREADS"))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
