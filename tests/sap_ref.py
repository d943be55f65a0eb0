"""numpy fp64 restatement of libdvae_sap_hip.so (include/dvae_sap_hip.h): the one-feature squared-hinge SVMs behind the
discrete-factor SAP score -- the objective of LinearSVC(C, class_weight="balanced"), the same Newton iteration on the active set,
the prediction rule, and a first-order bound on the coefficients.  A plain helper module (like mass_ref.py): no test in here.

The bound.  At the stopping point theta = (w, b) solves H theta = g with H = I + 2 [[Sxx, Sx], [Sx, S1]], g = 2 (Rx, R1), sums
over the active rows.  A sum of n terms accumulated in fp64 in any order is within n 2^-53 sum|terms| of the exact one, and the
one or two roundings of a term itself add 2 2^-53 sum|terms|: (S + 2) 2^-53 sum|terms| per sum.  To first order
    |d theta| <= ||H^-1|| (||dg|| + ||dH|| ||theta||) = B           (2-norms; dH by its Frobenius norm)
for the device and for this module alike.  A row ON the hinge belongs to either active set at no cost: its terms carry the
factor (1 - s (w x + b)) = 0.  The device is held to 4 B (the project's margin on first-order bounds).
"""
import numpy as np

U = 2.0 ** -53
MAX_ITERATIONS = 64
MAX_HALVINGS = 30


def problems_of(C):
    return C if C >= 3 else C - 1


def problem_list(n_classes):
    """[(factor j, class k)] in the order of coef's second index."""
    out = []
    for j, C in enumerate(n_classes):
        out += [(j, 1)] if C == 2 else [(j, k) for k in range(C if C >= 3 else 0)]
    return out


def weights(pos, Cj, C):
    """(c_+, c_-) of class_weight="balanced": S / (classes present * count), on the positives only unless the factor is binary."""
    S, n_pos = float(len(pos)), float(pos.sum())
    cp = C * (S / (float(Cj) * n_pos))
    cn = C * (S / (float(Cj) * (S - n_pos))) if Cj == 2 else C
    return cp, cn


def _sc(pos, cp, cn):
    return np.where(pos, 1.0, -1.0), np.where(pos, cp, cn)


def objective(x, pos, cp, cn, w, b):
    s, c = _sc(pos, cp, cn)
    m = s * (w * x + b)
    r = np.where(m < 1.0, 1.0 - m, 0.0)
    return 0.5 * (w * w + b * b) + float((c * r * r).sum())


def active(x, pos, w, b):
    return np.where(pos, 1.0, -1.0) * (w * x + b) < 1.0


def sums(x, pos, cp, cn, w, b):
    """(S1, Sx, Sxx, Rx, R1) over the rows active at (w, b)."""
    s, c = _sc(pos, cp, cn)
    a = active(x, pos, w, b)
    x, s, c = x[a], s[a], c[a]
    return float(c.sum()), float((c * x).sum()), float(((c * x) * x).sum()), float(((c * s) * x).sum()), float((c * s).sum())


def full_step(q):
    S1, Sx, Sxx, Rx, R1 = q
    a, h, e, rx, r1 = 1.0 + 2.0 * Sxx, 2.0 * Sx, 1.0 + 2.0 * S1, 2.0 * Rx, 2.0 * R1
    det = a * e - h * h
    return (e * rx - h * r1) / det, (a * r1 - h * rx) / det


def newton(x, pos, Cj, C, backtrack=True):
    """The device's recursion -> (w, b, iterations, halvings taken); iterations = -1 at the bound."""
    x = np.asarray(x, dtype=np.float64)
    cp, cn = weights(pos, Cj, C)
    w = b = 0.0
    f = objective(x, pos, cp, cn, w, b)
    halvings = 0
    for it in range(1, MAX_ITERATIONS + 1):
        wf, bf = full_step(sums(x, pos, cp, cn, w, b))
        if np.array_equal(active(x, pos, wf, bf), active(x, pos, w, b)):
            return wf, bf, it, halvings
        t, accepted = 1.0, False
        for hv in range(MAX_HALVINGS + 1):
            cw, cb = (wf, bf) if hv == 0 else (w + t * (wf - w), b + t * (bf - b))
            fc = objective(x, pos, cp, cn, cw, cb)
            if fc < f or not backtrack:
                accepted = True
                break
            t *= 0.5
            halvings += 1
        if not accepted:
            return w, b, it, halvings
        w, b, f = cw, cb, fc
    return w, b, -1, halvings


def gradient(x, pos, cp, cn, w, b):
    S1, Sx, Sxx, Rx, R1 = sums(x, pos, cp, cn, w, b)
    return np.array([w - 2.0 * (Rx - w * Sxx - b * Sx), b - 2.0 * (R1 - w * Sx - b * S1)])


def bound(x, pos, cp, cn, w, b):
    """(B, ||H||): the module docstring's bound at (w, b), and the 2-norm of H there."""
    x = np.asarray(x, dtype=np.float64)
    _s, c = _sc(pos, cp, cn)
    a = active(x, pos, w, b)
    ax, c = np.abs(x[a]), c[a]
    n = (len(x) + 2) * U
    d1, dx, dxx = n * c.sum(), n * (c * ax).sum(), n * (c * ax * ax).sum()
    S1, Sx, Sxx, _Rx, _R1 = sums(x, pos, cp, cn, w, b)
    H = np.array([[1.0 + 2.0 * Sxx, 2.0 * Sx], [2.0 * Sx, 1.0 + 2.0 * S1]])
    eig = np.linalg.eigvalsh(H)
    dH = 2.0 * np.sqrt(dxx * dxx + 2.0 * dx * dx + d1 * d1)
    dg = 2.0 * np.hypot(dx, d1)                                           # |c s x| = c |x|, |c s| = c
    return float((dg + dH * np.hypot(w, b)) / eig[0]), float(eig[-1])


def near_hinge(x, pos, w, b, B):
    """Does a row lie within the reach of a coefficient error B of the hinge s (w x + b) = 1?"""
    x = np.asarray(x, dtype=np.float64)
    m = np.where(pos, 1.0, -1.0) * (w * x + b)
    return bool((np.abs(1.0 - m) <= B * (np.abs(x) + 1.0) + 4 * U * (np.abs(w * x) + abs(b) + 1.0)).any())


def fit(table, rows, labels, n_classes, C):
    """-> coef [D, P, 2], iterations [D, P], halvings [D, P]."""
    D, plist = table.shape[1], problem_list(n_classes)
    coef, its, hv = np.zeros((D, len(plist), 2)), np.zeros((D, len(plist)), dtype=np.int32), np.zeros((D, len(plist)), dtype=np.int32)
    for d in range(D):
        x = table[rows, d].astype(np.float64)
        for p, (j, k) in enumerate(plist):
            coef[d, p, 0], coef[d, p, 1], its[d, p], hv[d, p] = newton(x, labels[j] == k, n_classes[j], C)
    return coef, its, hv


def decisions(wb, x):
    """[T, problems]: fl(fl(w x) + b), numpy rounds the product before the sum."""
    prod = x[:, None] * wb[None, :, 0]
    return prod + wb[None, :, 1]


def predict(wb, x, Cj):
    """int32 [T]: the arg-max (numpy's: the lowest class on ties), the sign test for two classes, class 0 for one."""
    if Cj >= 3:
        return decisions(wb, x).argmax(axis=1).astype(np.int32)
    if Cj == 2:
        return (decisions(wb, x)[:, 0] > 0.0).astype(np.int32)
    return np.zeros(len(x), dtype=np.int32)


def accuracy(table, rows, labels, n_classes, coef):
    """-> correct int32 [D, K], predicted int32 [D, K, T]; a label of -1 (a value never seen in training) is never met."""
    D, K, T = table.shape[1], len(n_classes), len(rows)
    correct, predicted = np.zeros((D, K), dtype=np.int32), np.zeros((D, K, T), dtype=np.int32)
    for d in range(D):
        x, p0 = table[rows, d].astype(np.float64), 0
        for j, Cj in enumerate(n_classes):
            predicted[d, j] = predict(coef[d, p0:p0 + problems_of(Cj)], x, Cj)
            correct[d, j] = (predicted[d, j] == labels[j]).sum()
            p0 += problems_of(Cj)
    return correct, predicted


def sap(score_matrix):
    """Mean over the factors of the largest minus the second largest entry over the latents (one latent: minus 0)."""
    m = np.sort(np.asarray(score_matrix, dtype=np.float64), axis=0)[::-1]
    return float(np.mean(m[0] - (m[1] if m.shape[0] > 1 else 0.0)))


# ---- tables and labels ----------------------------------------------------------------------------------------------------------------
FAMILIES = ("sharp", "noisy", "noise", "constant", "offset", "separable", "hinge")
# the hinge family: lat_sizes (3, 2), every column this one; on HINGE_ROWS (classes 0, 1, 0, 1, 2 of factor 0) the problem of class 0 at
# C = 0.5 has its optimum (-3 / 11, -1 / 11) with both positives exactly ON the hinge: the full step hops between the two pieces'
# minimisers, one point in exact arithmetic and two in fp64, and every halving of it fails to lower the objective
HINGE_COLUMN = (-4.0, -4.0, 3.0, 4.0, 4.0, 4.0)
HINGE_ROWS = (0, 2, 1, 3, 4)


def factor_values(rows, lat_sizes):
    """[K, S]: the digits of the row numbers of a data set that enumerates lat_sizes row-major."""
    rows = np.asarray(rows, dtype=np.int64)
    strides = [int(np.prod(lat_sizes[k + 1:])) for k in range(len(lat_sizes))]
    return np.stack([(rows // st) % size for st, size in zip(strides, lat_sizes)])


def table(family, lat_sizes, D, seed=0):
    """fp32 [prod(lat_sizes), D].  Column d follows factor d % K (its value / size), seen through: sharp -- 0.02 noise; noisy --
    noise as wide as the factor; noise -- nothing but N(0, 1); constant -- column 0 is 0.7 everywhere, the rest noisy; offset -- the
    project's 30 + 1e-3 (signal + noise); separable -- the factor's values 10 apart, 1e-2 noise (few active rows at the optimum)."""
    assert family in FAMILIES, family
    if family == "hinge":
        assert tuple(lat_sizes) == (3, 2)
        return np.repeat(np.array(HINGE_COLUMN, dtype=np.float32)[:, None], D, axis=1)
    N, K = int(np.prod(lat_sizes)), len(lat_sizes)
    rng = np.random.default_rng(7919 * seed + 31 * N + D + 1009 * FAMILIES.index(family))
    v = factor_values(np.arange(N), lat_sizes)
    signal = np.stack([v[d % K] / float(lat_sizes[d % K]) for d in range(D)], axis=1)
    noise = rng.standard_normal((N, D))
    if family == "sharp":
        out = signal + 0.02 * noise
    elif family == "noisy":
        out = signal + 0.5 * noise
    elif family == "noise":
        out = noise
    elif family == "constant":
        out = signal + 0.5 * noise
        out[:, 0] = 0.7
    elif family == "offset":
        out = 30.0 + 1e-3 * (signal + 0.3 * noise)
    else:
        out = 10.0 * np.stack([v[d % K] for d in range(D)], axis=1) + 1e-2 * noise
    return out.astype(np.float32)


def labels_of(train, test, lat_sizes):
    """(labels_train [K, S], labels_test [K, T] with -1 for unseen values, n_classes [K]): ranks among the values present in train."""
    vt, ve = factor_values(train, lat_sizes), factor_values(test, lat_sizes)
    lt, le, n = [], [], []
    for k in range(len(lat_sizes)):
        classes = np.unique(vt[k])
        n.append(len(classes))
        lt.append(np.searchsorted(classes, vt[k]))
        at = np.minimum(np.searchsorted(classes, ve[k]), len(classes) - 1)
        le.append(np.where(classes[at] == ve[k], at, -1))
    return np.stack(lt).astype(np.int32), np.stack(le).astype(np.int32), n


def reference(tab, lat_sizes, train, test, C=0.01):
    """Everything sap_discrete_from_table returns, from this module alone."""
    lt, le, n = labels_of(train, test, lat_sizes)
    coef, its, _hv = fit(tab, train, lt, n, C)
    ctrain, _ = accuracy(tab, train, lt, n, coef)
    ctest, _ = accuracy(tab, test, le, n, coef)
    m_train, m_test = ctrain / float(len(train)), ctest / float(len(test))
    return {"sap_discrete": sap(m_test), "score_matrix": m_test, "score_matrix_train": m_train, "coef": coef,
            "n_iterations_max": int(its.max()) if its.size else 0}


# ---- the end-to-end tables ------------------------------------------------------------------------------------------------------------
GRID = (3, 4, 5, 6)                                                           # 360 rows: 240 to fit, 120 to test


def end_to_end_tables():
    """fp32 [360, 6].  ideal: latent k holds factor k (the separable family) and two latents of noise; rotated: the four informative
    latents turned by a random orthogonal matrix, every one a mixture of all factors; collapsed: noise alone."""
    ideal = np.concatenate([table("separable", GRID, 4, seed=1), table("noise", GRID, 2, seed=2)], axis=1)
    q, _ = np.linalg.qr(np.random.default_rng(3).standard_normal((4, 4)))
    rotated = np.concatenate([(ideal[:, :4].astype(np.float64) @ q).astype(np.float32), ideal[:, 4:]], axis=1)
    return {"ideal": ideal, "rotated": rotated, "collapsed": table("noise", GRID, 6, seed=4)}


def end_to_end_rows():
    return np.random.default_rng(5).permutation(360)
