"""fp64 restatement (numpy) of the FactorVAE score (Kim & Mnih 2018, section 4) and the beta-VAE score (Higgins et al. 2017,
section 3) as disentanglement_lib's factor_vae.py / beta_vae.py define them, for the tests of Evaluator.compute_factor_scores:
written from the definitions, independent of the kernels of libdvae_score_hip.so and of disvae_amd/evaluate.py (its own row
drawing, its own classifier fit -- a damped Newton iteration on the same strictly convex objective)."""
import functools

import numpy as np


# ---- data --------------------------------------------------------------------------------------------------------------------
def strides(lat_sizes):
    return np.array([int(np.prod(lat_sizes[j + 1:])) for j in range(len(lat_sizes))], dtype=np.int64)


def factor_values(lat_sizes):
    """[N, K] int64: the value of every factor at every row of a data set that enumerates lat_sizes in row-major order."""
    n = int(np.prod(lat_sizes))
    return np.stack(np.unravel_index(np.arange(n), lat_sizes), axis=1).astype(np.int64)


@functools.lru_cache(maxsize=None)
def synthetic_table(lat_sizes, kind, seed=0):
    """fp32 [N, K + 2].  "ideal": dimension j < K is factor j scaled to [-1, 1] plus N(0, 0.02^2) noise, the last two dimensions
    N(0, 0.01^2) noise.  "rotated": the same with the first K dimensions multiplied by a fixed random orthogonal matrix.
    Cached: shared by the tests, never modified (the array is read-only)."""
    lat_sizes = tuple(int(k) for k in lat_sizes)
    K = len(lat_sizes)
    rng = np.random.default_rng(seed)
    vals = factor_values(lat_sizes).astype(np.float64)
    scaled = np.stack([2.0 * vals[:, j] / max(lat_sizes[j] - 1, 1) - 1.0 for j in range(K)], axis=1)
    z = np.concatenate([scaled + 0.02 * rng.standard_normal(scaled.shape), 0.01 * rng.standard_normal((len(vals), 2))], axis=1)
    if kind == "rotated":
        q, _ = np.linalg.qr(np.random.default_rng(1234).standard_normal((K, K)))
        z[:, :K] = z[:, :K] @ q
    else:
        assert kind == "ideal", kind
    out = z.astype(np.float32)
    out.setflags(write=False)
    return out


def draw_rows(lat_sizes, n_groups, batch_size, rng, paired=False):
    """The row drawing of the issue in numpy: (factor int32 [V], rows int64 [V, L]) or (factor, rows_a, rows_b)."""
    sizes = np.array(lat_sizes, dtype=np.int64)
    V, L = n_groups, batch_size
    eligible = np.nonzero(sizes >= 2)[0]
    factor = eligible[rng.integers(len(eligible), size=V)]
    a = rng.integers(0, sizes, size=(V, L, len(sizes)))
    st = strides(lat_sizes)
    idx = np.arange(V)
    if not paired:
        a[idx, :, factor] = rng.integers(0, sizes[factor])[:, None]
        return factor.astype(np.int32), (a * st).sum(-1)
    b = rng.integers(0, sizes, size=(V, L, len(sizes)))
    b[idx, :, factor] = a[idx, :, factor]
    return factor.astype(np.int32), (a * st).sum(-1), (b * st).sum(-1)


# ---- the statistics ------------------------------------------------------------------------------------------------------------
def group_var(table, rows, inv_scale=None):
    """[V, D] fp64: unbiased variance of table[rows[v, :], d] around the group's mean (times inv_scale[d])."""
    x = np.asarray(table, dtype=np.float64)[np.asarray(rows)]                # [V, L, D]
    dev = x - x.mean(axis=1, keepdims=True)
    var = (dev * dev).sum(axis=1) / (x.shape[1] - 1)
    return var if inv_scale is None else var * np.asarray(inv_scale, dtype=np.float64)


def pair_absdiff(table, rows_a, rows_b):
    t = np.asarray(table, dtype=np.float64)
    return np.abs(t[np.asarray(rows_a)] - t[np.asarray(rows_b)]).mean(axis=1)


def vote(stat, factor, active, K):
    """argmin [V] (the active d with the smallest statistic, lowest index on ties, never a NaN, -1 when there is none) and the
    votes [K, D] -- written as the plain loops of the definition."""
    stat = np.asarray(stat)
    V, D = stat.shape
    argmin = np.full(V, -1, dtype=np.int32)
    votes = np.zeros((K, D), dtype=np.int32)
    for v in range(V):
        best = -1
        for d in range(D):
            x = stat[v, d]
            if active[d] and not np.isnan(x) and (best < 0 or x < stat[v, best]):
                best = d
        argmin[v] = best
        if best >= 0:
            votes[factor[v], best] += 1
    return argmin, votes


def near_ties(stat, active, rel=1e-4):
    """bool [V]: groups whose smallest and second-smallest active statistics differ by less than `rel` relative (a group with
    fewer than two usable statistics has no tie)."""
    s = np.where(np.asarray(active, dtype=bool)[None, :], np.asarray(stat, dtype=np.float64), np.nan)
    s = np.sort(s, axis=1)                                                  # NaN last
    if s.shape[1] < 2:
        return np.zeros(len(s), dtype=bool)
    lo, hi = s[:, 0], s[:, 1]
    with np.errstate(invalid="ignore"):
        return np.isfinite(lo) & np.isfinite(hi) & ((hi - lo) < rel * np.abs(hi))


def factor_vae_from_votes(votes_train, votes_eval, n_train, n_eval):
    classifier = np.argmax(votes_train, axis=0)
    return (float(votes_train.max(axis=0).sum()) / n_train,
            float(votes_eval[classifier, np.arange(votes_train.shape[1])].sum()) / n_eval)


# ---- the classifier ------------------------------------------------------------------------------------------------------------
def logreg_loss_grad(W, b, X, y, C=1.0):
    """mean cross-entropy + ||W||^2 / (2 C n), bias unpenalised: (loss, dW, db, softmax probabilities)."""
    n = len(X)
    logits = X @ W.T + b
    logits -= logits.max(axis=1, keepdims=True)
    p = np.exp(logits)
    p /= p.sum(axis=1, keepdims=True)
    loss = -np.log(p[np.arange(n), y]).mean() + (W * W).sum() / (2.0 * C * n)
    g = p.copy()
    g[np.arange(n), y] -= 1.0
    return loss, g.T @ X / n + W / (C * n), g.mean(axis=0), p


def fit_logreg(X, y, n_classes, C=1.0, tol=1e-10, max_iter=200):
    """Damped Newton on the objective of logreg_loss_grad from zero (the Hessian's null space -- a common shift of the biases --
    is left to the least-squares solve)."""
    X = np.asarray(X, dtype=np.float64)
    n, D = X.shape
    Xa = np.concatenate([X, np.ones((n, 1))], axis=1)                        # bias as a last, unpenalised feature
    P = n_classes * (D + 1)
    theta = np.zeros((n_classes, D + 1))
    reg = np.ones((n_classes, D + 1)) / (C * n)
    reg[:, D] = 0.0
    for _ in range(max_iter):
        loss, dW, db, p = logreg_loss_grad(theta[:, :D], theta[:, D], X, y, C)
        g = np.concatenate([dW, db[:, None]], axis=1)
        if np.abs(g).max() < tol:
            break
        H = np.zeros((n_classes, D + 1, n_classes, D + 1))
        for i in range(n_classes):
            for j in range(n_classes):
                w = p[:, i] * ((i == j) - p[:, j])
                H[i, :, j, :] = (Xa * w[:, None]).T @ Xa / n
        H = H.reshape(P, P) + np.diag(reg.reshape(P))
        step = np.linalg.lstsq(H, g.reshape(P), rcond=None)[0].reshape(theta.shape)
        t = 1.0
        while t > 1e-10:
            cand = theta - t * step
            if logreg_loss_grad(cand[:, :D], cand[:, D], X, y, C)[0] <= loss - 1e-4 * t * (g * step).sum():
                break
            t *= 0.5
        theta = theta - t * step
    return theta[:, :D].copy(), theta[:, D].copy()


def accuracy(W, b, classes, X, y):
    return float((classes[np.argmax(np.asarray(X, dtype=np.float64) @ W.T + b, axis=1)] == y).mean())


# ---- the two scores ------------------------------------------------------------------------------------------------------------
def make_draws(lat_sizes, n_train, n_eval, batch_size, n_variance, seed):
    """Every draw of one run, in numpy: the dict factor_scores_from_table(draws=...) takes (after torch.from_numpy)."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(lat_sizes))
    return {"variance_rows": rng.permutation(n)[:min(n, n_variance)],
            "factor_vae_train": draw_rows(lat_sizes, n_train, batch_size, rng),
            "factor_vae_eval": draw_rows(lat_sizes, n_eval, batch_size, rng),
            "beta_vae_train": draw_rows(lat_sizes, n_train, batch_size, rng, paired=True),
            "beta_vae_eval": draw_rows(lat_sizes, n_eval, batch_size, rng, paired=True)}


def scores(table, lat_sizes, draws, active_threshold=0.05):
    """Both scores in fp64 on the given draws; returns (scores, details) as factor_scores_from_table(return_details=True)."""
    K = len(lat_sizes)
    var = group_var(table, draws["variance_rows"][None, :])[0]
    active = np.sqrt(var) >= active_threshold
    det = {"var": var, "active": active}
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / var
        for key in ("train", "eval"):
            factor, rows = draws["factor_vae_" + key]
            det["stat_" + key] = group_var(table, rows, inv)
            det["argmin_" + key], det["votes_" + key] = vote(det["stat_" + key], factor, active, K)
    n_train, n_eval = len(draws["factor_vae_train"][0]), len(draws["factor_vae_eval"][0])
    fv_train, fv_eval = factor_vae_from_votes(det["votes_train"], det["votes_eval"], n_train, n_eval)
    for key in ("train", "eval"):
        factor, rows_a, rows_b = draws["beta_vae_" + key]
        det["features_" + key], det["labels_" + key] = pair_absdiff(table, rows_a, rows_b), factor.astype(np.int64)
    classes = np.unique(det["labels_train"])
    W, b = fit_logreg(det["features_train"], np.searchsorted(classes, det["labels_train"]), len(classes))
    det.update(W=W, b=b, classes=classes)
    out = {"factor_vae_train": fv_train, "factor_vae_eval": fv_eval,
           "beta_vae_train": accuracy(W, b, classes, det["features_train"], det["labels_train"]),
           "beta_vae_eval": accuracy(W, b, classes, det["features_eval"], det["labels_eval"]),
           "n_active": int(active.sum()), "n_train": n_train, "n_eval": n_eval, "batch_size": draws["factor_vae_train"][1].shape[1]}
    return out, det
