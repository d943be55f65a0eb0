"""numpy-only fp64 restatement of the model of include/dvae_dci_hip.h -- scikit-learn's GradientBoostingClassifier() as version
1.7 implements it: log loss, depth-3 friedman_mse regression trees on the residuals, a Newton step per leaf, impurity-based
importances -- and of disentanglement_lib's DCI scores on top of it.  A plain helper module (like udr_ref.py).

* ``fit``            the model: tree dump in the library's layout (feature [n_stages, T, 15], stats [n_stages, T, 15, 5] =
                     threshold, value, n, sum r, sum r^2; heap order), raw scores, importances;
* ``candidates`` / ``best_split``   the VERIFIER: given a node's rows and the residuals, the gain of every legal (feature,
                     threshold) and the best one (lowest feature, then lowest position among exactly equal gains);
* ``partition_gap``  the relative gap between the best and the second-best DISTINCT partition of a node;
* ``verify``         replays a dump -- the library's or ``fit``'s own -- stage by stage and checks every node against the verifier.

Sums here are numpy's (pairwise); the library adds in the fixed order its header states.  The two differ in the last bits, which
can decide between splits of (nearly) equal gain: that is why a dump is verified, not compared.
"""
import numpy as np

EPS = float(np.finfo(np.float64).eps)
FEATURE_THRESHOLD = np.float32(1e-7)
NODES, STATS = 15, 5
PRIOR_EPS = float(np.finfo(np.float32).eps)


def trees(C):
    return 1 if C <= 2 else int(C)


def prior(labels, C):
    q = np.clip(np.bincount(labels, minlength=C)[:C] / float(len(labels)), PRIOR_EPS, 1 - PRIOR_EPS)
    if C == 1:
        return np.zeros(1)
    if C == 2:
        return np.array([np.log(q[1] / (1 - q[1]))])
    return np.log(q / np.exp(np.mean(np.log(q))))


def targets(labels, C):
    """y [T, S]"""
    if C == 2:
        return labels.astype(np.float64)[None]
    return (labels[None, :] == np.arange(trees(C))[:, None]).astype(np.float64)


def residuals(raw, labels, C):
    """r [T, S] from the raw scores [S, T] before the stage"""
    if C == 2:
        return targets(labels, C) - (1.0 / (1.0 + np.exp(-raw[:, 0])))[None]
    e = np.exp(raw - raw.max(axis=1, keepdims=True))
    return targets(labels, C) - (e / e.sum(axis=1, keepdims=True)).T


def mse(n, sr, srr):
    m = sr / n
    return srr / n - m * m


def threshold_of(lo, hi):
    thr = float(lo) / 2.0 + float(hi) / 2.0
    return float(lo) if (thr == float(hi) or np.isinf(thr)) else thr


def candidates(X, r, members, d):
    """The legal splits of the node holding rows ``members`` (ascending row numbers) on feature d, in the order of their
    positions: -> (gain, lo, hi, n_left) arrays.  A position is legal when the value exceeds that of the node's row before it in
    the stable ascending order by more than 1e-7 in fp32."""
    x = X[members, d]
    o = np.argsort(x, kind="stable")
    xs, rs = x[o], r[members][o]
    ok = xs[1:] > (xs[:-1] + FEATURE_THRESHOLD)                          # fp32 + fp32
    nl = np.arange(1, len(members), dtype=np.float64)[ok]
    sl = np.cumsum(rs)[:-1][ok]
    nr, sr = len(members) - nl, np.cumsum(r[members])[-1] - sl           # ONE total per node, whatever the feature
    diff = nr * sl - nl * sr
    return diff * diff / (nl * nr), xs[:-1][ok], xs[1:][ok], nl.astype(np.int64)


def best_split(X, r, members):
    """-> (feature, threshold, gain) of the best legal split, or (-1, 0.0, -1.0): the largest gain, among exactly equal gains the
    lowest feature, then the lowest position."""
    best = (-1, 0.0, -1.0)
    for d in range(X.shape[1]):
        gain, lo, hi, _nl = candidates(X, r, members, d)
        if len(gain):
            i = int(np.argmax(gain))                                     # the first of equal maxima
            if gain[i] > best[2]:
                best = (d, threshold_of(lo[i], hi[i]), float(gain[i]))
    return best


_ROW_KEYS = np.random.default_rng(12345).integers(0, 2 ** 63, size=1 << 15, dtype=np.uint64)     # one random word per row


def partition_gap(X, r, members):
    """(best - second best) / best over the DISTINCT partitions the legal splits of the node induce; 1.0 with one partition or
    none, 0.0 when the best gain is 0.  A partition is known by the sum (mod 2^64) of the random words of the rows of a side --
    the left side of a candidate is a prefix of the sorted column, so a cumulative sum gives them all; the smaller of the two
    sides' sums stands for both orientations."""
    keys = _ROW_KEYS[members]
    whole = keys.sum(dtype=np.uint64)
    gains, sides = [], []
    for d in range(X.shape[1]):
        gain, _lo, _hi, nl = candidates(X, r, members, d)
        left = np.cumsum(keys[np.argsort(X[members, d], kind="stable")], dtype=np.uint64)[nl - 1]
        gains.append(gain)
        sides.append(np.minimum(left, whole - left))
    gains, sides = np.concatenate(gains), np.concatenate(sides)
    if len(gains) == 0:
        return 1.0
    o = np.argsort(sides, kind="stable")
    starts = np.flatnonzero(np.r_[True, sides[o][1:] != sides[o][:-1]])
    top = np.sort(np.maximum.reduceat(gains[o], starts))[::-1][:2]      # the best gain of every distinct partition
    if len(top) < 2:
        return 1.0
    return float((top[0] - top[1]) / top[0]) if top[0] > 0 else 0.0


def node_sums(r, y, members):
    rr = r[members]
    p = y[members] - rr
    return float(len(members)), float(rr.sum()), float((rr * rr).sum()), float((p * (1 - p)).sum())


def leaf_value(n, sr, sh, C):
    num = sr / n * (1.0 if C == 2 else (C - 1.0) / C)
    den = sh / n
    return 0.0 if abs(den) < 1e-150 else num / den


def fit_tree(X, r, y, C, gaps=None):
    """One depth-3 tree on the residuals r -> (feature [15], stats [15, 5], node of every row)."""
    S = X.shape[0]
    feature, stats = np.full(NODES, -1, np.int32), np.zeros((NODES, STATS))
    node = np.zeros(S, np.int64)
    members = {0: np.arange(S)}
    for h in range(NODES):
        if h not in members:
            continue
        m = members[h]
        n, sr, srr, sh = node_sums(r, y, m)
        stats[h, 2:] = n, sr, srr
        f = -1
        if h < 7 and n >= 2 and mse(n, sr, srr) > EPS:
            f, thr, _gain = best_split(X, r, m)
        if f < 0:
            stats[h, 1] = leaf_value(n, sr, sh, C)
            continue
        if gaps is not None:
            gaps.append(partition_gap(X, r, m))
        feature[h], stats[h, 0], stats[h, 1] = f, thr, sr / n
        left = X[m, f].astype(np.float64) <= thr
        members[2 * h + 1], members[2 * h + 2] = m[left], m[~left]
        node[m[left]], node[m[~left]] = 2 * h + 1, 2 * h + 2
    return feature, stats, node


def tree_importance(feature, stats, D):
    """per-feature importance of one dumped tree: sum over its inner nodes of (n mse - nL mseL - nR mseR) / n_root"""
    imp = np.zeros(D)
    for h in range(7):
        if feature[h] >= 0:
            own, l, r = stats[h, 2:], stats[2 * h + 1, 2:], stats[2 * h + 2, 2:]
            imp[feature[h]] += own[0] * mse(*own) - l[0] * mse(*l) - r[0] * mse(*r)
    return imp / stats[0, 2]


def importance_of_dump(feature, stats, D):
    """-> (sum over the trees in order [D], number of trees that split)"""
    total, n_split = np.zeros(D), 0
    for f, s in zip(feature.reshape(-1, NODES), stats.reshape(-1, NODES, STATS)):
        total += tree_importance(f, s, D)
        n_split += int(f[0] >= 0)
    return total, n_split


def normalised_importance(total, n_split):
    """GradientBoostingClassifier.feature_importances_: the mean over the trees that split, normalised; zeros when none did"""
    if n_split == 0 or total.sum() == 0:
        return np.zeros_like(total)
    avg = total / n_split
    return avg / avg.sum()


def fit(X, labels, C, n_stages, learning_rate=0.1, raw=None, gaps=False):
    """X fp32 [S, D], labels int [S] in [0, C).  raw: continue from these raw scores [S, T] (None: from the prior).
    -> {"feature", "stats", "raw", "importance" [D] (summed), "n_split", "gaps" (one per split node)}"""
    assert X.dtype == np.float32
    S, D = X.shape
    T = trees(C)
    labels = np.asarray(labels, np.int64)
    raw = np.tile(prior(labels, C), (S, 1)) if raw is None else np.array(raw, np.float64)
    y = targets(labels, C)
    feature, stats = np.zeros((n_stages, T, NODES), np.int32), np.zeros((n_stages, T, NODES, STATS))
    gap_list = [] if gaps else None
    for i in range(n_stages):
        r = residuals(raw, labels, C)
        for k in range(T):
            feature[i, k], stats[i, k], node = fit_tree(X, r[k], y[k], C, gap_list)
            raw[:, k] += learning_rate * stats[i, k, node, 1]
    total, n_split = importance_of_dump(feature, stats, D)
    return {"feature": feature, "stats": stats, "raw": raw, "importance": total, "n_split": n_split, "gaps": gap_list}


def predict(X, feature, stats, raw, learning_rate=0.1):
    """raw [S, T] (the prior) plus the dumped trees, stage by stage"""
    raw = np.array(raw, np.float64)
    Xd = X.astype(np.float64)
    for i in range(feature.shape[0]):
        for k in range(feature.shape[1]):
            h = np.zeros(len(X), np.int64)
            for _depth in range(3):
                f = feature[i, k, h]
                go = f >= 0
                right = Xd[np.arange(len(X)), np.maximum(f, 0)] > stats[i, k, h, 0]
                h = np.where(go, 2 * h + 1 + right, h)
            raw[:, k] += learning_rate * stats[i, k, h, 1]
    return raw


def classes_of(raw, C):
    return (raw[:, 0] > 0).astype(np.int64) if C == 2 else np.argmax(raw, axis=1)


def verify(X, labels, C, feature, stats, raw_after, learning_rate=0.1, raw_before=None):
    """Replays a tree dump and checks every node of every tree against the verifier, whatever happened at ties:
      - n, sum r and sum r^2 of the node's rows (from the dump's OWN thresholds) within 8 S 2^-53 sum |r| of the dumped ones;
      - a leaf above depth 3 has n < 2, mse <= eps (on the dumped sums, to the rounding of that expression) or no legal split;
      - a split is a legal candidate -- feature, threshold bits -- of a gain >= (1 - 1e-10) x the best gain of the node, and
        both children are non-empty;
      - values within 1e-12 relative of the verifier's: f (sum r / n) / (sum h / n) of a leaf, sum r / n of an inner node, with
        the DUMPED sum r -- itself held to its bound above; the residuals of a node can cancel (the root's add up to rounding
        noise), so a quotient of the verifier's own sum r would not be a number to be relative to -- over the verifier's n and
        sum h (positive terms: no cancellation);
      - every entry of raw_after within 1e-12 relative of the replay (which starts from raw_before, or from the verifier's prior).
    -> {"nodes": split nodes, "other_choice": how many of them differ from best_split's own choice, "worst_sum", "worst_value"}."""
    S, D = X.shape
    T = trees(C)
    labels = np.asarray(labels, np.int64)
    raw = np.tile(prior(labels, C), (S, 1)) if raw_before is None else np.array(raw_before, np.float64)
    y = targets(labels, C)
    out = {"nodes": 0, "other_choice": 0, "worst_sum": 0.0, "worst_value": 0.0}
    for i in range(feature.shape[0]):
        r = residuals(raw, labels, C)
        for k in range(T):
            members = {0: np.arange(S)}
            node = np.zeros(S, np.int64)
            for h in range(NODES):
                where = "stage %d tree %d node %d" % (i, k, h)
                f, (thr, value, n, sr, srr) = int(feature[i, k, h]), stats[i, k, h]
                if h not in members:
                    assert f == -1 and not stats[i, k, h].any(), where + ": a node that does not exist is not all zero"
                    continue
                m = members[h]
                vn, vsr, vsrr, vsh = node_sums(r[k], y[k], m)
                bound = 8 * S * 2.0 ** -53 * np.abs(r[k][m]).sum()
                assert n == vn, where + ": n"
                assert abs(sr - vsr) <= bound and abs(srr - vsrr) <= bound, (where, sr - vsr, srr - vsrr, bound)
                if bound > 0:
                    out["worst_sum"] = max(out["worst_sum"], abs(sr - vsr) / bound, abs(srr - vsrr) / bound)
                slack = 4 * 2.0 ** -53 * srr / n                           # rounding of srr / n - (sr / n)^2, with or without an fma
                if f < 0:
                    assert thr == 0.0, where
                    if h < 7 and n >= 2 and mse(n, sr, srr) > EPS + slack:
                        assert best_split(X, r[k], m)[0] < 0, where + ": a leaf that has a legal split"
                    want = leaf_value(vn, sr, vsh, C)                      # the DUMPED sum r (checked above) over the verifier's sum h
                else:
                    assert h < 7 and n >= 2 and mse(n, sr, srr) > EPS - slack and 0 <= f < D, where + ": split of a node that is a leaf"
                    gain, lo, hi, _nl = candidates(X, r[k], m, f)
                    at = [j for j in range(len(gain)) if threshold_of(lo[j], hi[j]) == thr]
                    assert at, where + ": the threshold is no legal candidate of feature %d" % f
                    bf, bthr, bgain = best_split(X, r[k], m)
                    assert gain[at[0]] >= (1 - 1e-10) * bgain, (where, gain[at[0]], bgain)
                    out["nodes"] += 1
                    out["other_choice"] += int((bf, bthr) != (f, thr))
                    left = X[m, f].astype(np.float64) <= thr
                    assert left.any() and not left.all(), where
                    members[2 * h + 1], members[2 * h + 2] = m[left], m[~left]
                    node[m[left]], node[m[~left]] = 2 * h + 1, 2 * h + 2
                    want = sr / vn
                assert abs(value - want) <= 1e-12 * abs(want), (where, value, want)
                if want != 0:
                    out["worst_value"] = max(out["worst_value"], abs(value - want) / abs(want))
            raw[:, k] += learning_rate * stats[i, k, node, 1]             # the dump's own values: errors do not pile up
    assert (np.abs(raw - raw_after) <= 1e-12 * np.abs(raw)).all(), np.abs(raw - raw_after).max()
    assert out["worst_value"] <= 1e-12
    return out


# ---- disentanglement_lib's dci.py on the importance matrix ---------------------------------------------------------------------
def _entropy(p, base):
    p = p[p > 0]
    return float(-(p * np.log(p)).sum() / np.log(base))


def dci_scores(importance):
    """importance [D, K] -> (disentanglement, completeness) with disentanglement_lib's formulas"""
    R = np.asarray(importance, np.float64)
    D, K = R.shape
    per_code = np.array([1.0 - _entropy((R[d] + 1e-11) / (R[d] + 1e-11).sum(), K) for d in range(D)])
    per_factor = np.array([1.0 - _entropy((R[:, k] + 1e-11) / (R[:, k] + 1e-11).sum(), D) for k in range(K)])
    if R.sum() == 0.0:
        code_w, factor_w = np.ones(D) / D, np.ones(K) / K
    else:
        code_w, factor_w = R.sum(axis=1) / R.sum(), R.sum(axis=0) / R.sum()
    return float((per_code * code_w).sum()), float((per_factor * factor_w).sum())


# ---- seeded tables the CPU and the GPU tests share ---------------------------------------------------------------------------------
def table(S, D, C, seed, kind="mixed"):
    """X fp32 [S, D], labels [S].  "mixed": column 0 informative, column 1 rounded to 1 / 2 (ties), column 2 constant (D >= 3), the
    rest noise; "clean": one strongly informative continuous column, nothing tied; "pure": class 0 is exactly the rows with
    column 0 below every other row's, so a depth-1 node turns pure while its sibling goes on; "overlap": as "clean" with classes that
    overlap, so that no node turns pure."""
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, C, S)
    labels[:C] = np.arange(C)                                            # every class is present
    X = rng.standard_normal((S, D))
    if kind == "pure":
        X[:, 0] = np.where(labels == 0, -5.0, 0.0) + rng.random(S) + 0.3 * labels
        if D > 1:
            X[:, 1] = labels + 0.8 * rng.standard_normal(S)
    else:
        X[:, 0] = labels + (0.15 if kind == "clean" else 0.6) * rng.standard_normal(S)
    if kind == "overlap":                                                # classes that overlap, nothing tied: no node turns pure
        X[:, 0] = labels + 0.6 * rng.standard_normal(S)
    if kind == "mixed":
        if D > 1:
            X[:, 1] = np.round((0.5 * labels + rng.standard_normal(S)) * 2) / 2
        if D > 2:
            X[:, 2] = 0.25
    return X.astype(np.float32), labels.astype(np.int64)


# name -> (S, D, C, n_stages, kind): the smallest shapes at which each piece of the library can go wrong.  A thread of the library
# owns ceil(S / 1024) consecutive rows, so 1024 | 1025 is its one switch; D = 1 and D = 5 are one feature and a number of them
# that no power of two divides.  CAP_CASES are the ones on which test_dci_host.py finds the best-vs-second-best gap of the
# restatement >= 1e-9 on 98 % of the split nodes or more: there the library's own choices may differ from best_split's on 2 % of
# the nodes at the most.  The others hold nodes that are pure but for the rounding of their sums (every split of such a node has a
# gain of rounding noise) or mirror-image splits of equal gain: they are verified like the rest, without the cap.
CASES = {
    "narrowest": (96, 4, 3, 1, "mixed"),
    "basic": (96, 4, 3, 5, "mixed"),
    "two_class": (96, 4, 2, 5, "mixed"),
    "two_class_clean": (96, 4, 2, 5, "clean"),
    "five_class": (300, 6, 5, 10, "mixed"),
    "chunk_below": (1024, 5, 3, 2, "mixed"),
    "chunk_above": (1025, 5, 3, 2, "mixed"),
    "one_feature": (96, 1, 3, 3, "clean"),
    "pure": (96, 4, 3, 3, "pure"),
    "clean": (96, 4, 3, 1, "clean"),
    "large_lds": (4097, 2, 3, 1, "mixed"),                               # 13 bytes x 5 rows x 1024 threads: more than 64 KB of LDS
    "chunk_above_clean": (1025, 5, 3, 2, "clean"),                       # the far side of the switch, and the large sizes, on tables
    "large_lds_overlap": (4097, 2, 3, 1, "overlap"),                     # whose gaps allow the cap
    "max_rows": (10240, 2, 3, 1, "overlap"),                             # DVAE_DCI_MAX_ROWS: a thread owns 10 rows
}
CAP_CASES = ("basic", "two_class", "two_class_clean", "five_class", "chunk_below", "clean", "chunk_above_clean", "large_lds_overlap",
             "max_rows")


def case(name):
    """-> (X fp32 [S, D], labels [S], C, n_stages) of a named case"""
    S, D, C, n_stages, kind = CASES[name]
    X, labels = table(S, D, C, 1000 * S + 10 * D + C, kind)
    return X, labels, C, n_stages
