"""A numpy-only restatement of the k-nearest-neighbour mutual information between a continuous and a discrete variable (Ross
2014; include/dvae_knn_hip.h states it; scikit-learn's sklearn.feature_selection._mutual_info._compute_mi_cd is the same function)
and of the scores combined from its [latent, factor] matrix.  A plain helper module, like sap_ref.py; no scipy, no scikit-learn:
``digamma`` is passed in as a table psi[0 .. S] (tests/test_knn_host.py builds it from scipy where it compares with
scikit-learn, the GPU tests hand over the table the device got).

Two statements of the integers.  ``neighbours`` works on sorted lists (the class lists: a window of 2 k + 1 places holds the k
nearest; the full list: a vectorised bisection on exact fp64 differences); ``neighbours_brute`` forms every |x_j - x_i| and counts,
for small tables.  The tests hold the two to each other and the first to scikit-learn.
"""
import numpy as np


def factor_strides(lat_sizes):
    return [int(np.prod(lat_sizes[k + 1:])) for k in range(len(lat_sizes))]


def factor_values(rows, lat_sizes):
    """int64 [K, S]: the value of every factor in every row number."""
    rows = np.asarray(rows, dtype=np.int64)
    return np.stack([(rows // s) % n for s, n in zip(factor_strides(lat_sizes), lat_sizes)])


def class_sizes(v):
    """c_i of every row: the number of rows with its label."""
    _vals, inverse, counts = np.unique(v, return_inverse=True, return_counts=True)
    return counts[inverse]


def neighbours_brute(x, v, kn):
    """(keep bool [S], k_i, c_i, m_i int64 [S], 0 for dropped rows) from all pairwise fp64 distances."""
    x = np.asarray(x).astype(np.float64)
    v = np.asarray(v)
    c = class_sizes(v)
    keep = c >= 2
    k_i, m_i = np.zeros(len(x), dtype=np.int64), np.zeros(len(x), dtype=np.int64)
    dist = np.abs(x[:, None] - x[None, :])
    for i in np.nonzero(keep)[0]:
        same = np.nonzero((v == v[i]) & keep)[0]
        others = np.sort(dist[i, same[same != i]])
        k_i[i] = min(kn, c[i] - 1)
        r = others[k_i[i] - 1]
        m_i[i] = (dist[i, keep] < r).sum() if r > 0 else (dist[i, keep] == 0).sum()
    return keep, k_i, np.where(keep, c, 0), m_i


def neighbours(x, v, kn):
    """The same integers from sorted lists."""
    x = np.asarray(x).astype(np.float64)
    v = np.asarray(v)
    S = len(x)
    c = class_sizes(v)
    keep = c >= 2
    k_i, m_i, radius = np.zeros(S, dtype=np.int64), np.zeros(S, dtype=np.int64), np.zeros(S)
    k_i[keep] = np.minimum(kn, c[keep] - 1)
    for label in np.unique(v[keep]):
        members = np.nonzero(v == label)[0]
        members = members[np.argsort(x[members], kind="stable")]
        a, kk = x[members], int(k_i[members[0]])
        padded = np.concatenate([np.full(kk, np.inf), a, np.full(kk, np.inf)])
        window = np.stack([padded[o:o + len(a)] for o in range(2 * kk + 1)], axis=1)       # places i - kk .. i + kk of the class list
        dist = np.sort(np.abs(window - a[:, None]), axis=1)
        radius[members] = dist[:, kk]                                    # place 0 is the row itself
    kept = np.nonzero(keep)[0]
    xs = np.sort(x[kept])
    n = len(xs)
    if n:
        xi, ri = x[kept], radius[kept]
        at = np.searchsorted(xs, xi, side="left")                        # a place of the value x_i

        def inside(dist):
            return np.where(ri > 0, dist < ri, dist <= 0)
        lo, hi = np.zeros(len(kept), dtype=np.int64), at.copy()           # the first place inside: in [lo, hi]
        while (lo < hi).any():
            mid = (lo + hi) // 2
            ok = inside(xi - xs[mid])
            go = lo < hi
            hi = np.where(go & ok, mid, hi)
            lo = np.where(go & ~ok, mid + 1, lo)
        first = lo
        lo, hi = at.copy(), np.full(len(kept), n - 1, dtype=np.int64)     # the last place inside: in [lo, hi]
        while (lo < hi).any():
            mid = (lo + hi + 1) // 2
            ok = inside(xs[mid] - xi)
            go = lo < hi
            lo = np.where(go & ok, mid, lo)
            hi = np.where(go & ~ok, mid - 1, hi)
        m_i[kept] = lo - first + 1
    return keep, k_i, np.where(keep, c, 0), m_i


def estimate(x, v, kn, psi, brute=False):
    """The estimator on one column -> dict(n, k_i, c_i, m_i, sums (sum psi(k), sum psi(c), sum psi(m)), terms (the three arrays
    of psi values over the kept rows), raw, mi).  psi: a table with psi[j] = digamma(j), j >= 1."""
    psi = np.asarray(psi, dtype=np.float64)
    keep, k_i, c_i, m_i = (neighbours_brute if brute else neighbours)(x, v, kn)
    n = int(keep.sum())
    terms = [psi[k_i[keep]], psi[c_i[keep]], psi[m_i[keep]]]
    if n == 0:
        return dict(n=0, k_i=k_i, c_i=c_i, m_i=m_i, sums=np.zeros(3), terms=terms, raw=0.0, mi=0.0)
    raw = psi[n] + np.mean(terms[0]) - np.mean(terms[1]) - np.mean(terms[2])
    return dict(n=n, k_i=k_i, c_i=c_i, m_i=m_i, sums=np.array([t.sum() for t in terms]), terms=terms, raw=float(raw), mi=max(0.0, float(raw)))


def raw_from_sums(n, sums, psi):
    """psi(n) + (sum psi(k) - sum psi(c) - sum psi(m)) / n from the device's outputs, 0 where n == 0: [D, K]."""
    n = np.asarray(n, dtype=np.int64)
    sums = np.asarray(sums, dtype=np.float64)
    safe = np.maximum(n, 1)
    raw = np.asarray(psi)[safe] + sums[..., 0] / safe - sums[..., 1] / safe - sums[..., 2] / safe
    return np.where(n > 0, raw, 0.0)


def factor_entropy(counts):
    p = np.asarray(counts, dtype=np.float64)
    p = p[p > 0] / p.sum()
    return float(-(p * np.log(p)).sum())


def gap(m, axis):
    ranked = -np.sort(-m, axis=axis)
    top = np.take(ranked, 0, axis=axis)
    return top - (np.take(ranked, 1, axis=axis) if m.shape[axis] > 1 else 0.0)


def scores(raw, H):
    """The scores from the raw [D, K] matrix and the factor entropies [K] (nats)."""
    raw, H = np.asarray(raw, dtype=np.float64), np.asarray(H, dtype=np.float64)
    mi = np.maximum(raw, 0.0)
    D, K = mi.shape
    nmi = mi / H[None, :]
    sq = mi ** 2
    t = sq.max(axis=1)
    modularity = np.zeros(D)
    for d in range(D):
        if t[d] > 0:
            modularity[d] = 1.0 - (sq[d].sum() - t[d]) / (t[d] * (K - 1)) if K > 1 else 1.0
    prefers = mi.argmax(axis=1)
    gap_d = gap(mi, 1)
    dcimig = sum(gap_d[prefers == k].max() for k in range(K) if (prefers == k).any()) / H.sum()
    active = [d for d in range(D) if (mi[d] != 0).any()]
    Da = len(active)
    infom = infoc = 0.0
    if Da:
        per_d = [1.0 if K == 1 else (nmi[d].max() / nmi[d].sum() - 1.0 / K) / (1.0 - 1.0 / K) for d in active]
        cols = [k for k in range(K) if (mi[:, k] != 0).any()]
        per_k = [1.0 if Da == 1 else (nmi[active, k].max() / nmi[active, k].sum() - 1.0 / Da) / (1.0 - 1.0 / Da) for k in cols]
        infom, infoc = float(np.mean(per_d)), float(np.mean(per_k))
    return dict(mig=float(np.mean(gap(mi, 0) / H)), mig_sup=float(np.mean(gap(nmi, 1))), dcimig=float(dcimig),
                modularity=float(modularity.mean()), infom=infom, infoc=infoc, n_active=Da, best_latent=mi.argmax(axis=0))


# ---- tables ---------------------------------------------------------------------------------------------------------------------------
def table(family, lat_sizes, D, seed=0):
    """fp32 [prod(lat_sizes), D] tables built to break a sort-and-search.  Column d follows factor d % K where the family has a
    signal."""
    rng = np.random.default_rng(seed)
    N, K = int(np.prod(lat_sizes)), len(lat_sizes)
    vals = factor_values(np.arange(N), lat_sizes)
    centred = np.stack([vals[d % K] / max(lat_sizes[d % K] - 1, 1) * 4.0 - 2.0 for d in range(D)], axis=1)
    noise = rng.standard_normal((N, D))
    if family == "clusters":
        tab = centred + 0.3 * noise
    elif family == "noise":
        tab = noise
    elif family == "constant":                                           # column 0 constant, the rest clusters
        tab = centred + 0.3 * noise
        tab[:, 0] = 1.25
    elif family == "grid":                                               # values on a 2^-3 grid: equal distances left and right
        tab = np.round((centred + 0.5 * noise) * 8.0) / 8.0
    elif family == "zeros":                                              # +0, -0 and a few values around them
        tab = np.round(centred * 0.5 + 0.4 * noise)
        tab = np.where(tab == 0, np.where(rng.random((N, D)) < 0.5, 0.0, -0.0), tab)
    elif family == "denormal":                                           # multiples of the smallest fp32 denormal
        tab = (np.round((centred + 0.5 * noise) * 16.0) * 2.0 ** -149)
    elif family == "offset":                                             # 30 + 1e-3 noise
        tab = 30.0 + 1e-3 * (centred + 0.3 * noise)
    elif family == "ulp":                                                # values that differ only in the lowest mantissa bits
        steps = np.round((centred + 0.5 * noise) * 2.0).astype(np.int64) + 16
        tab = (np.float32(1.0).view(np.int32) + steps).astype(np.int32).view(np.float32).astype(np.float64)
    else:
        raise ValueError(family)
    return np.ascontiguousarray(tab.astype(np.float32))


def reference(tab, lat_sizes, rows, kn, psi):
    """Every (latent, factor) pair of tab[rows]: dict(n [D, K], sums [D, K, 3], bound [D, K, 3] (sum |psi terms| of each sum),
    raw [D, K], m_i / k_i [D, K, S], counts (list of K arrays))."""
    rows = np.asarray(rows, dtype=np.int64)
    D, K, S = tab.shape[1], len(lat_sizes), len(rows)
    vals = factor_values(rows, lat_sizes)
    out = dict(n=np.zeros((D, K), dtype=np.int64), sums=np.zeros((D, K, 3)), bound=np.zeros((D, K, 3)), raw=np.zeros((D, K)),
               m_i=np.zeros((D, K, S), dtype=np.int64), k_i=np.zeros((D, K, S), dtype=np.int64),
               counts=[np.bincount(vals[k], minlength=lat_sizes[k]) for k in range(K)])
    for d in range(D):
        for k in range(K):
            e = estimate(tab[rows, d], vals[k], kn, psi)
            out["n"][d, k], out["sums"][d, k], out["raw"][d, k] = e["n"], e["sums"], e["raw"]
            out["bound"][d, k] = [np.abs(t).sum() for t in e["terms"]]
            out["m_i"][d, k], out["k_i"][d, k] = e["m_i"], e["k_i"]
    return out
