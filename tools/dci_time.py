"""Cost of the boosted-tree kernels (libdvae_dci_hip.so, csrc/boosted_trees.hip) and of the whole dci_from_table at the dSprites
shape -- 10 000 training rows of a [737 280, 10] table, factors with 3 / 6 / 40 / 32 / 32 values, 100 stages -- next to the only
alternative without them: scikit-learn's GradientBoostingClassifier().fit on the same rows on this machine's CPU.

The table is synthetic: latent k follows factor k (noise of a third of a step), the other five latents are noise.  Device events
around each dvae_dci_fit, `--reps` repeats after a warm-up, the median and the spread.  A stage is DVAE_DCI_LAUNCHES_PER_STAGE
dependent launches; "floor_ms" is the same call on 256 rows of the same table, where the work of every kernel is negligible and
what remains is the launches, the gaps between them and the fixed cost of the workgroups: floor / median is an UPPER estimate
of the share of the fit that is launch gaps.  scikit-learn (--sklearn): the 3-class factor in full, the others for --sklearn-stages stages
and multiplied up (marked "extrapolated").  Prints one JSON line per measurement and writes them to --out.

    python tools/dci_time.py [--reps 5] [--sklearn] [--out profiles/dci_time.jsonl]
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

from disvae_amd import _dcilib  # noqa: E402
from disvae_amd._lib import ptr  # noqa: E402
from disvae_amd.engine import _stream  # noqa: E402
from disvae_amd.evaluate import DCI_LEARNING_RATE, dci_from_table  # noqa: E402

LAT_SIZES, D, N_TRAIN, N_TEST, STAGES = (3, 6, 40, 32, 32), 10, 10000, 5000, 100


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
    return round(times[len(times) // 2], 3), [round(times[0], 3), round(times[-1], 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sklearn", action="store_true")
    ap.add_argument("--sklearn-stages", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dci_time.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is nothing to time without it"
    lines = []

    def emit(what, **more):
        lines.append(json.dumps(dict({"what": what, "D": D, "n_train": N_TRAIN, "stages": STAGES}, **more)))
        print(lines[-1], flush=True)

    n = int(np.prod(LAT_SIZES))
    gen = torch.Generator(device="cuda").manual_seed(1)
    idx = torch.arange(n, device="cuda")
    mean = torch.randn(n, D, generator=gen, device="cuda")
    strides = [int(np.prod(LAT_SIZES[k + 1:])) for k in range(len(LAT_SIZES))]
    for k, size in enumerate(LAT_SIZES):
        mean[:, k] = ((idx // strides[k]) % size).float() + mean[:, k] / 3
    mean = mean.contiguous()
    rows = torch.randperm(n, generator=gen, device="cuda")[:N_TRAIN + N_TEST].contiguous()
    h = _dcilib.lib()
    st = _stream()

    def fitter(train, values, C):
        S, T = int(train.numel()), _dcilib.trees(C)
        order = torch.sort(mean.index_select(0, train), dim=0, stable=True).indices.t().contiguous().to(torch.int32)
        labels = values.to(torch.int32).contiguous()
        buf = {"ws": torch.empty(h.dvae_dci_fit_ws_floats(n, D, S, C, STAGES), device="cuda"),
               "raw": torch.empty(S, T, dtype=torch.float64, device="cuda"), "prior": torch.empty(T, dtype=torch.float64, device="cuda"),
               "imp": torch.empty(D, dtype=torch.float64, device="cuda"),
               "n_split": torch.empty(1, dtype=torch.int32, device="cuda"),
               "feature": torch.empty(STAGES, T, _dcilib.NODES, dtype=torch.int32, device="cuda"),
               "stats": torch.empty(STAGES, T, _dcilib.NODES, _dcilib.NODE_STATS, dtype=torch.float64, device="cuda")}

        def fit():
            _dcilib.call("dvae_dci_fit", ptr(mean), ptr(train), ptr(order), ptr(labels), n, D, S, C, STAGES, DCI_LEARNING_RATE, 1,
                         ptr(buf["raw"]), ptr(buf["prior"]), ptr(buf["ws"]), ptr(buf["imp"]), ptr(buf["n_split"]), ptr(buf["feature"]), ptr(buf["stats"]), st)
        return fit, buf

    train = rows[:N_TRAIN].contiguous()
    importances = {}
    for k, C in enumerate(LAT_SIZES):
        values = (train // strides[k]) % C
        fit, buf = fitter(train, values, C)
        t = median_ms(fit, args.reps)
        floor_fit, _ = fitter(train[:256].contiguous(), values[:256], C)
        floor = median_ms(floor_fit, args.reps)
        total = buf["imp"].cpu().numpy()
        importances[k] = total / total.sum()
        launches = STAGES * _dcilib.LAUNCHES_PER_STAGE + 3
        emit("dvae_dci_fit", factor=k, classes=C, trees=STAGES * _dcilib.trees(C), reps=args.reps, median_ms=t[0], spread_ms=t[1],
             launches=launches, launches_per_stage=_dcilib.LAUNCHES_PER_STAGE, floor_ms=floor[0], floor_spread_ms=floor[1],
             launch_gap_share=round(floor[0] / t[0], 3), us_per_launch=round(1000 * t[0] / launches, 2))

    def whole():
        return dci_from_table(mean, LAT_SIZES, n_train=N_TRAIN, n_test=N_TEST, rows=rows, n_stages=STAGES)
    whole()
    walls = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = whole()
        torch.cuda.synchronize()
        walls.append(1000 * (time.perf_counter() - t0))
    walls.sort()
    emit("dci_from_table", n_test=N_TEST, reps=args.reps, median_ms=round(walls[len(walls) // 2], 2),
         spread_ms=[round(walls[0], 2), round(walls[-1], 2)],
         **{key: round(got[key], 4) for key in ("disentanglement", "completeness", "informativeness_train", "informativeness_test")})

    if args.sklearn:
        from sklearn.ensemble import GradientBoostingClassifier
        X = mean.index_select(0, train).cpu().numpy()
        for k, C in enumerate(LAT_SIZES):
            y = ((train // strides[k]) % C).cpu().numpy()
            stages = STAGES if C == 3 else args.sklearn_stages
            t0 = time.perf_counter()
            model = GradientBoostingClassifier(n_estimators=stages, random_state=0).fit(X, y)
            seconds = time.perf_counter() - t0
            emit("sklearn GradientBoostingClassifier.fit", factor=k, classes=C, stages_timed=stages, seconds_timed=round(seconds, 2),
                 seconds_100_stages=round(seconds * STAGES / stages, 1), extrapolated=stages != STAGES,
                 cpu_threads_env=os.environ.get("OMP_NUM_THREADS"),
                 importance_max_abs_difference=(round(float(np.abs(model.feature_importances_ - importances[k]).max()), 6)
                                                if stages == STAGES else None))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
