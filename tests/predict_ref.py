"""numpy-only restatement of the host half of the prediction-based scores (downstream task, fairness, explicitness): the
aggregates, the unfairness of a count matrix, the one-vs-rest AUC from scores with the tie-averaged ranks written out, and the
row arithmetic of an intervention.  Nothing here imports the package; the tests hold disvae_amd.evaluate to it and it to
scikit-learn."""
import numpy as np


def strides(lat_sizes):
    return [int(np.prod(lat_sizes[k + 1:])) for k in range(len(lat_sizes))]


def factor_table(lat_sizes):
    """int64 [N, K]: the factor values of every row of a data set that enumerates lat_sizes row-major, written out."""
    grids = np.meshgrid(*[np.arange(k) for k in lat_sizes], indexing="ij")
    return np.stack(grids, axis=-1).reshape(-1, len(lat_sizes)).astype(np.int64)


def intervened(base, lat_sizes, j):
    """int64 [size_j, P]: for every value c of factor j the row number of `base` with factor j set to c -- through the explicit
    factor table, not through the strides."""
    factors = factor_table(lat_sizes)
    lookup = {tuple(f): r for r, f in enumerate(factors)}
    out = np.zeros((lat_sizes[j], len(base)), np.int64)
    for c in range(lat_sizes[j]):
        for p, r in enumerate(base):
            f = factors[int(r)].copy()
            f[j] = c
            out[c, p] = lookup[tuple(f)]
    return out


# ---- the fixture tables of the tests --------------------------------------------------------------------------------------------
SMALL, LARGE, DIM = (3, 4, 5), (4, 6, 8, 5), 6                           # N = 60 and N = 960


def ideal_table(lat_sizes, seed=0, noise=0.2):
    """fp32 [N, DIM]: latent k is factor k plus uniform noise in (-noise, noise) -- below half a step, and below a quarter: the
    midpoint between any two neighbouring values' rows separates ALL their rows --, the other latents are N(0, 1) noise."""
    rng = np.random.default_rng(seed)
    factors = factor_table(lat_sizes)
    z = rng.standard_normal((len(factors), DIM))
    z[:, :len(lat_sizes)] = factors + rng.uniform(-noise, noise, factors.shape)
    return z.astype(np.float32)


def entangled_table(lat_sizes, seed=0):
    """fp32 [N, DIM]: latent 0 is v_0 + size_0 v_1 (it tells factor 0 AND factor 1), the other latents are N(0, 1) noise."""
    rng = np.random.default_rng(seed)
    factors = factor_table(lat_sizes)
    z = rng.standard_normal((len(factors), DIM))
    z[:, 0] = factors[:, 0] + lat_sizes[0] * factors[:, 1]
    return z.astype(np.float32)


def drawn_rows(n, count, seed):
    """`count` distinct row numbers of n, int64"""
    return np.random.default_rng(seed).permutation(n)[:count].astype(np.int64)


# ---- downstream task ---------------------------------------------------------------------------------------------------------
def downstream_keys(sizes, K):
    keys = set()
    for n in sizes:
        for name in ("train", "test"):
            keys |= {"%d:mean_%s_accuracy" % (n, name), "%d:min_%s_accuracy" % (n, name)}
            keys |= {"%d:%s_accuracy_factor_%d" % (n, name, k) for k in range(K)}
        if n != max(sizes):
            keys.add("%d:efficiency" % n)
    return keys


def downstream_aggregates(sizes, acc_train, acc_test):
    """acc_*: [len(sizes), K]"""
    out = {}
    for i, n in enumerate(sizes):
        for name, acc in (("train", np.asarray(acc_train, np.float64)[i]), ("test", np.asarray(acc_test, np.float64)[i])):
            out["%d:mean_%s_accuracy" % (n, name)] = float(np.sum(acc) / len(acc))
            out["%d:min_%s_accuracy" % (n, name)] = float(min(acc))
            for k in range(len(acc)):
                out["%d:%s_accuracy_factor_%d" % (n, name, k)] = float(acc[k])
    top = out["%d:mean_test_accuracy" % max(sizes)]
    for n in sizes:
        if n != max(sizes):
            out["%d:efficiency" % n] = out["%d:mean_test_accuracy" % n] / top if top > 0 else 0.0
    return out


# ---- fairness ----------------------------------------------------------------------------------------------------------------
def counts_of(predicted, classes):
    """predicted: the predicted VALUES [size_j, P]; classes: the values present in training -> counts [C, size_j]"""
    classes = [int(c) for c in classes]
    counts = np.zeros((len(classes), predicted.shape[0]), np.int64)
    for c in range(predicted.shape[0]):
        for v in predicted[c]:
            counts[classes.index(int(v)), c] += 1
    return counts


def unfairness(counts):
    """(mean, max) over the columns of the total variation between a column's distribution and the overall one"""
    counts = np.asarray(counts, np.float64)
    total = counts.sum()
    overall = counts.sum(axis=1) / total
    tvs, weights = [], []
    for c in range(counts.shape[1]):
        n_c = counts[:, c].sum()
        if n_c == 0:
            continue
        p = counts[:, c] / n_c
        tvs.append(0.5 * np.abs(p - overall).sum())
        weights.append(n_c)
    tvs, weights = np.array(tvs), np.array(weights)
    return float((tvs * weights).sum() / weights.sum()), float(tvs.max())


def fairness_aggregates(mean_m, max_m):
    K = mean_m.shape[0]
    off = [(i, j) for i in range(K) for j in range(K) if i != j]
    return {"mean_unfairness": float(np.mean([mean_m[ij] for ij in off])), "max_unfairness": float(np.mean([max_m[ij] for ij in off])),
            "mean_unfairness_per_target": np.array([sum(mean_m[i, j] for j in range(K) if j != i) / (K - 1) for i in range(K)]),
            "mean_unfairness_per_sensitive": np.array([sum(mean_m[i, j] for i in range(K) if i != j) / (K - 1) for j in range(K)])}


# ---- explicitness ------------------------------------------------------------------------------------------------------------
def average_ranks(x):
    """1-based tie-averaged ranks of a vector, written out: a sort, then every run of equal values gets (first + last) / 2 + 1"""
    x = np.asarray(x)
    order = np.argsort(x, kind="stable")
    ranks = np.zeros(len(x), np.float64)
    first = 0
    while first < len(x):
        last = first
        while last + 1 < len(x) and x[order[last + 1]] == x[order[first]]:
            last += 1
        ranks[order[first:last + 1]] = (first + last) / 2.0 + 1.0
        first = last + 1
    return ranks


def binary_auc(scores, positive):
    """(R+ - n+ (n+ + 1) / 2) / (n+ n-); NaN without positives or without negatives"""
    positive = np.asarray(positive, bool)
    n_pos, n_neg = float(positive.sum()), float((~positive).sum())
    if n_pos == 0 or n_neg == 0:
        return float("nan")
    r_pos = float(average_ranks(scores)[positive].sum())
    return (r_pos - n_pos * (n_pos + 1.0) / 2.0) / (n_pos * n_neg)


def ovr_auc(prob, labels):
    """prob [S, C] (fp32 as it was ranked), labels [S] in [-1, C) -> (per-class AUC [C], their mean over the classes that have
    positives and negatives; NaN when there is none)"""
    prob, labels = np.asarray(prob), np.asarray(labels)
    auc = np.array([binary_auc(prob[:, v], labels == v) for v in range(prob.shape[1])])
    ok = ~np.isnan(auc)
    return auc, (float(np.mean(auc[ok])) if ok.any() else float("nan"))
