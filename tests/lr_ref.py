"""fp64 numpy restatement of include/dvae_lr_hip.h (a plain helper module, like sap_ref.py): the objective of the multinomial
logistic regression, its gradient and FULL Hessian (P = C (D + 1) is small on every test table), a damped Newton solve on the
subspace sum_c b_c = 0 to max |grad| <= 1e-13 (the reference optimum theta*), the device's truncated Newton-CG restated step for
step (its iteration counts, for the head-room test), the first-order rounding bounds of what the device adds, and the tables.

theta is ONE vector in the layout of `coef`: W [C, D] row-major, then b [C].

THE BOUNDS (u = 2^-53; first order in u; every sum in the order the header states).
  logit      z_ic = b_c + sum_d W_cd x_id, D fused multiply-adds in ascending d:   |dz_ic| <= zeta_ic = (D + 1) u (|b_c| + sum_d |W_cd| |x_id|),
             zeta_i = max_c zeta_ic.  x_id itself is the same fp64 number on both sides (fl(fl(x - shift) scale), two roundings here as there).
  softmax    e_c = exp(z_c - m), m = max z (exp to 2 u):  relative eps_ic = 2 zeta_i + u |z_ic - m_i| + 2 u;  the sum of C terms adds (C - 1) u and
             its relative error is the p-weighted mean of eps; the division adds u:  dp_ic = p_ic (eps_ic + sum_c' p_ic' eps_ic' + (C + 1) u).
  gradient   G_cd = (sum over chunks, in chunk order, of (sum over the chunk's L rows, in row order, of r_ic x_id)) / S + W_cd / (C S),
             r = p - y (one rounding: u |r|).  A term passes at most L + n_chunks additions:
             B_g(c, d) = (u / S) ((L + n_chunks + 1) sum_i |r_ic| |x_id| + sum_i |x_id| dp_ic / u) + 3 u |W_cd| / (C S) + 2 u |G_cd|
             and B_g = max over the entries.  The same expression with r = p (u - s) bounds a Hessian-vector product; it is not needed here.
  objective  loss_i = (m - z_y) + log(sum e):  |dloss_i| <= 2 zeta_i + sum_c p_ic eps_ic + (C + 4) u (|m - z_y| + |log sum e| + 1);
             thread t adds rows t, t + 512, ..., then 6 shuffle steps and 8 waves:  n_add = ceil(S / 512) + 6 + 8;
             B_f = (n_add u sum_i |loss_i| + sum_i |dloss_i|) / S + 2 u |f| + (C D / 512 + 17) u ||W||^2 / (2 C S).
  log_loss   of dvae_lr_predict, 128 threads and 2 waves: n_add = ceil(T / 128) + 6 + 2;  B = n_add u sum_i |loss_i| + sum_i |dloss_i|.
"""
import functools

import numpy as np

U = 2.0 ** -53
THREADS, CHUNK_ROWS, PREDICT_THREADS = 512, 64, 128
MAX_ITERATIONS, MAX_CG, MAX_HALVINGS = 100, 400, 30


# ---- the objective ------------------------------------------------------------------------------------------------------------------
def features(X32, shift=None, scale=None):
    """The fp64 features the device forms: (double) x, or fl(fl(x - shift) scale)."""
    X = np.asarray(X32, dtype=np.float32).astype(np.float64)
    if shift is None:
        return X
    return (X - np.asarray(shift, dtype=np.float64)[None, :]) * np.asarray(scale, dtype=np.float64)[None, :]


def split(theta, C, D):
    theta = np.asarray(theta, dtype=np.float64)
    return theta[:C * D].reshape(C, D), theta[C * D:]


def join(W, b):
    return np.concatenate([np.asarray(W, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)])


def centred(theta, C, D):
    """theta with mean(b) taken off b: the point of the same objective on sum b = 0."""
    W, b = split(theta, C, D)
    return join(W, b - b.mean())


def logits(X, theta, C):
    W, b = split(theta, C, X.shape[1])
    return X @ W.T + b[None, :]


def softmax(Z):
    m = Z.max(axis=1, keepdims=True)
    E = np.exp(Z - m)
    s = E.sum(axis=1, keepdims=True)
    return E / s, m[:, 0], s[:, 0]


def row_losses(X, y, theta, C):
    Z = logits(X, theta, C)
    _P, m, s = softmax(Z)
    return (m - Z[np.arange(len(y)), y]) + np.log(s)


def objective(X, y, C, reg_C, theta):
    W, _b = split(theta, C, X.shape[1])
    S = X.shape[0]
    return float(row_losses(X, y, theta, C).sum() / S + (W * W).sum() / (2.0 * reg_C * S))


def _residual(X, y, theta, C):
    P, _m, _s = softmax(logits(X, theta, C))
    R = P.copy()
    R[np.arange(len(y)), y] -= 1.0
    return P, R


def gradient(X, y, C, reg_C, theta):
    S, D = X.shape
    W, _b = split(theta, C, D)
    _P, R = _residual(X, y, theta, C)
    return join(R.T @ X / S + W / (reg_C * S), R.sum(axis=0) / S)


def hessian_vector(X, P, C, reg_C, v):
    S, D = X.shape
    V, vb = split(v, C, D)
    Uv = X @ V.T + vb[None, :]
    R = P * (Uv - (P * Uv).sum(axis=1, keepdims=True))
    return join(R.T @ X / S + V / (reg_C * S), R.sum(axis=0) / S)


def hessian_diagonal(X, P, C, reg_C):
    """The diagonal of the Hessian in theta's layout: the preconditioner of the device's conjugate gradients."""
    S = X.shape[0]
    w = P * (1.0 - P)
    return join(w.T @ (X * X) / S + 1.0 / (reg_C * S), w.sum(axis=0) / S)


def hessian(X, y, C, reg_C, theta):
    """The full [P, P] Hessian in theta's layout."""
    S, D = X.shape
    P, _R = _residual(X, y, theta, C)
    X1 = np.concatenate([X, np.ones((S, 1))], axis=1)                       # [S, D + 1]
    H4 = np.zeros((C, D + 1, C, D + 1))
    for d in range(D + 1):
        for e in range(d, D + 1):
            w = X1[:, d] * X1[:, e]
            block = (np.diag((P * w[:, None]).sum(axis=0)) - (P * w[:, None]).T @ P) / S      # [C, C]: sum_i w_i (diag(p_i) - p_i p_i^T)
            H4[:, d, :, e] = block
            H4[:, e, :, d] = block
    idx = np.array([c * D + d if d < D else C * D + c for c in range(C) for d in range(D + 1)])
    H = np.zeros((C * (D + 1),) * 2)
    H[np.ix_(idx, idx)] = H4.reshape(C * (D + 1), C * (D + 1))
    H[np.arange(C * D), np.arange(C * D)] += 1.0 / (reg_C * S)
    return H


def null_vector(C, D):
    n = np.zeros(C * (D + 1))
    n[C * D:] = 1.0 / np.sqrt(C)
    return n


def pinv_norm(H, C, D):
    """||H^+||_inf, H^+ the pseudo-inverse on sum b = 0: (H + n n^T)^-1 - n n^T."""
    n = null_vector(C, D)
    return float(np.abs(np.linalg.inv(H + np.outer(n, n)) - np.outer(n, n)).sum(axis=1).max())


def newton(X, y, C, reg_C, tol=1e-13, max_iter=200):
    """Damped Newton from 0 on sum b = 0 -> (theta*, iterations, max |grad|)."""
    S, D = X.shape
    theta = np.zeros(C * (D + 1))
    n = null_vector(C, D)
    f, g = objective(X, y, C, reg_C, theta), gradient(X, y, C, reg_C, theta)
    for it in range(max_iter + 1):
        if np.abs(g).max() <= tol:
            return theta, it, float(np.abs(g).max())
        step = np.linalg.solve(hessian(X, y, C, reg_C, theta) + np.outer(n, n), -g)
        step -= n * (n @ step)
        t, best = 1.0, None
        for _h in range(60):
            cand = theta + t * step
            fc, gc = objective(X, y, C, reg_C, cand), gradient(X, y, C, reg_C, cand)
            if fc <= f + 1e-4 * t * (g @ step) or (fc <= f + 1e-12 * abs(f) and np.abs(gc).max() < np.abs(g).max()):
                best = (cand, fc, gc)
                break
            t *= 0.5
        if best is None:                                                     # the gradient is at its rounding floor
            return theta, it, float(np.abs(g).max())
        theta, f, g = best
        theta = centred(theta, C, D)
    return theta, -1, float(np.abs(g).max())


def newton_cg(X, y, C, reg_C, tol):
    """The device's iteration (include/dvae_lr_hip.h), with numpy's sums -> (theta, f, max |g|, iterations or -1, evaluations,
    conjugate-gradient steps in all)."""
    S, D = X.shape
    theta = np.zeros(C * (D + 1))
    f, g = objective(X, y, C, reg_C, theta), gradient(X, y, C, reg_C, theta)
    n_eval, n_cg = 1, 0
    for it in range(MAX_ITERATIONS + 1):
        gmax = float(np.abs(g).max())
        if gmax <= tol:
            return theta, f, gmax, it, n_eval, n_cg
        if it == MAX_ITERATIONS:
            break
        P, _R = _residual(X, y, theta, C)
        diag = hessian_diagonal(X, P, C, reg_C)
        diag[C * D:] = diag[C * D:].sum() / C                                # ONE number for the biases: the steps stay on sum b = 0
        minv = np.where(diag > 0, 1.0 / np.where(diag > 0, diag, 1.0), 1.0)
        s, res, p = np.zeros_like(g), -g, -g * minv
        gnorm = float(np.sqrt(g @ g))
        cg_tol, rz = min(0.5, np.sqrt(gnorm)) * gnorm, float((g * g) @ minv)
        for j in range(MAX_CG):
            hp = hessian_vector(X, P, C, reg_C, p)
            n_cg += 1
            curv = float(p @ hp)
            if not curv > 0.0:
                if j == 0:
                    s = res * minv
                break
            alpha = rz / curv
            s = s + alpha * p
            res = res - alpha * hp
            if np.sqrt(float(res @ res)) <= cg_tol:
                break
            rz_new = float((res * res) @ minv)
            p = res * minv + (rz_new / rz) * p
            rz = rz_new
        slope, t, accepted = float(g @ s), 1.0, None
        for _h in range(MAX_HALVINGS + 1):
            cand = theta + t * s
            fc, gc = objective(X, y, C, reg_C, cand), gradient(X, y, C, reg_C, cand)
            n_eval += 1
            if fc <= f + 1e-4 * t * slope or (fc <= f + 1e-12 * abs(f) and np.abs(gc).max() < gmax):
                accepted = (cand, fc, gc)
                break
            t *= 0.5
        if accepted is None:
            break
        theta, f, g = accepted
    return theta, f, float(np.abs(g).max()), -1, n_eval, n_cg


# ---- the bounds ---------------------------------------------------------------------------------------------------------------------
def chunks(S, C, D):
    """(n_chunks, rows of a chunk) of the device's sums over the rows: the header's plan."""
    per = max(THREADS // (C * (D + 1)), 1)
    nb = min((S + CHUNK_ROWS - 1) // CHUNK_ROWS, per)
    chunk = (S + nb - 1) // nb
    return (S + chunk - 1) // chunk, chunk


def _row_errors(X, y, theta, C):
    """(P, zeta [S], eps [S, C], dp [S, C], loss [S], dloss [S]) of the module docstring."""
    S, D = X.shape
    W, b = split(theta, C, D)
    Z = logits(X, theta, C)
    P, m, s = softmax(Z)
    zeta = ((D + 1) * U * (np.abs(b)[None, :] + np.abs(X) @ np.abs(W).T)).max(axis=1)
    eps = 2.0 * zeta[:, None] + U * np.abs(Z - m[:, None]) + 2.0 * U
    dp = P * (eps + (P * eps).sum(axis=1, keepdims=True) + (C + 1) * U)
    zy = Z[np.arange(S), np.clip(y, 0, C - 1)]
    loss = (m - zy) + np.log(s)
    dloss = 2.0 * zeta + (P * eps).sum(axis=1) + (C + 4) * U * (np.abs(m - zy) + np.abs(np.log(s)) + 1.0)
    return P, zeta, eps, dp, loss, dloss


def bound_gradient(X, y, C, reg_C, theta):
    """B_g at theta."""
    S, D = X.shape
    W, _b = split(theta, C, D)
    n_chunks, L = chunks(S, C, D)
    P, _zeta, _eps, dp, _loss, _dloss = _row_errors(X, y, theta, C)
    R = P.copy()
    R[np.arange(S), y] -= 1.0
    X1 = np.abs(np.concatenate([X, np.ones((S, 1))], axis=1))
    terms = (np.abs(R).T @ X1) * (L + n_chunks + 1) + (dp / U).T @ X1                              # [C, D + 1]
    G = np.abs(gradient(X, y, C, reg_C, theta))
    Gm = np.concatenate([G[:C * D].reshape(C, D), G[C * D:].reshape(C, 1)], axis=1)
    pen = np.concatenate([np.abs(W), np.zeros((C, 1))], axis=1) / (reg_C * S)
    return float((U / S * terms + 3.0 * U * pen + 2.0 * U * Gm).max())


def bound_objective(X, y, C, reg_C, theta):
    """B_f at theta."""
    S, D = X.shape
    W, _b = split(theta, C, D)
    _P, _zeta, _eps, _dp, loss, dloss = _row_errors(X, y, theta, C)
    n_add = -(-S // THREADS) + 6 + THREADS // 64
    f = abs(objective(X, y, C, reg_C, theta))
    return float((n_add * U * np.abs(loss).sum() + dloss.sum()) / S + 2.0 * U * f + (C * D / THREADS + 17) * U * (W * W).sum() / (2.0 * reg_C * S))


def predict(X, labels, theta, C):
    """dvae_lr_predict restated -> dict(prob fp64 [T, C], log_loss, bound (of log_loss), correct, counted, predicted [T], gap [T]: the
    top-two logit gap of every row, dz [T]: the bound zeta of a logit of the row)."""
    T = X.shape[0]
    labels = np.asarray(labels)
    P, zeta, _eps, _dp, loss, dloss = _row_errors(X, labels, theta, C)
    Z = logits(X, theta, C)
    seen = labels >= 0
    pred = Z.argmax(axis=1)                                                  # the lowest class on ties
    top = np.sort(Z, axis=1)
    gap = top[:, -1] - top[:, -2] if C >= 2 else np.full(T, np.inf)
    n_add = -(-T // PREDICT_THREADS) + 6 + PREDICT_THREADS // 64
    return dict(prob=P, log_loss=float(loss[seen].sum()), bound=float(n_add * U * np.abs(loss[seen]).sum() + dloss[seen].sum()),
                correct=int((pred == labels).sum()), counted=int(seen.sum()), predicted=pred, gap=gap, dz=zeta)


# ---- the tables ---------------------------------------------------------------------------------------------------------------------
FAMILIES = ("gauss", "aligned", "offset", "constant", "duplicates", "single")


def table(family, S, T, D, classes, seed):
    """-> (X fp32 [S + T, D], labels int32 [Q, S + T]) of a family; the first S rows train.  Every class of every problem occurs
    among the training rows.
      gauss       N(0, 1) features, labels drawn uniformly (nothing to learn: the penalty and the bias decide)
      aligned     feature q % D is the label of problem q plus noise below a quarter of a step: linearly separable, the penalty alone
                  keeps the optimum finite (the ill-conditioned case)
      offset      30 + 1e-3 (gauss + 0.5 label of problem 0): every column nearly collinear with the bias
      constant    gauss with the last column constant (0 when D == 1 ... the column is the only one: then all zeros)
      duplicates  gauss rows, each drawn WITH repeats from S // 3 + 1 distinct ones (labels go with the rows)
      single      gauss, and class 0 of every problem has exactly ONE training row"""
    rng = np.random.default_rng(seed)
    N = S + T
    labels = np.stack([rng.integers(0, C, N) for C in classes]).astype(np.int32)
    for q, C in enumerate(classes):                                          # every class among the training rows
        assert S >= C, (S, C)
        labels[q, rng.permutation(S)[:C]] = np.arange(C)
    X = rng.standard_normal((N, D))
    if family == "aligned":
        X *= 0.3
        for q in range(len(classes)):
            X[:, q % D] = labels[q] + rng.uniform(-0.2, 0.2, N)
    elif family == "offset":
        X = 30.0 + 1e-3 * (X + 0.5 * labels[0][:, None])
    elif family == "constant":
        X[:, -1] = 0.0
    elif family == "duplicates":
        pick = rng.integers(0, S // 3 + 1, N)
        X, labels = X[pick], labels[:, pick]
        for q, C in enumerate(classes):
            labels[q, :C] = np.arange(C)
    elif family == "single":
        for q, C in enumerate(classes):
            lab = labels[q, :S]
            lab[lab == 0] = 1 % C
            lab[int(rng.integers(0, S))] = 0
            for c in range(C):                                               # a class the line above removed comes back
                if not (lab == c).any():
                    free = np.flatnonzero((lab != 0) & (np.bincount(lab, minlength=C)[lab] > 1))
                    lab[free[0]] = c
    else:
        assert family == "gauss", family
    return np.ascontiguousarray(X, dtype=np.float32), np.ascontiguousarray(labels, dtype=np.int32)


def standardizer(X32, S):
    """(shift, scale) fp64 [D] of the first S rows: the column mean and 1 / population std, 0 for a constant column."""
    X = np.asarray(X32[:S], dtype=np.float64)
    mean, std = X.mean(axis=0), X.std(axis=0)
    return mean, np.where(std > 0, 1.0 / np.where(std > 0, std, 1.0), 0.0)


@functools.lru_cache(maxsize=None)
def solved(family, S, T, D, classes, seed, scaled, reg_C):
    """The inputs of a case and the reference optimum of every problem, computed once and shared."""
    X32, labels = table(family, S, T, D, classes, seed)
    shift, scale = standardizer(X32, S) if scaled else (None, None)
    if family == "constant" and scaled and D > 1:
        X32[:, -1] = 5.0                                                     # a constant that is not 0: scale 0 makes it one
        shift, scale = standardizer(X32, S)
        assert scale[-1] == 0.0
    X = features(X32, shift, scale)
    problems = []
    for q, C in enumerate(classes):
        theta, its, gmax = newton(X[:S], labels[q, :S], C, reg_C)
        problems.append(dict(theta=theta, iterations=its, gmax=gmax))
    return dict(X32=X32, labels=labels, shift=shift, scale=scale, X=X, problems=problems)


# The cases of tests/test_gpu_lr.py (tests/test_lr_host.py holds their reference solves to the head-room under the iteration bound):
# (name, family, training rows S, test rows T, D, classes of the Q problems, seed, shift / scale given, C)
# S = 2; 63 / 64 / 65 around DVAE_LR_CHUNK_ROWS; 511 / 512 / 513 around DVAE_LR_THREADS; DVAE_LR_MAX_ROWS once (D = 2, two classes);
# D = 1, 10, 17 (two feature tiles, the second ragged), 64 (four); 2, 3, 40 and 256 classes (256 at S = 512, D = 2: P = 768 entries, more
# than the threads); Q = 1, 5, 8 with mixed classes.
CASES = [
    ("rows-2", "gauss", 2, 5, 1, (2,), 1, False, 1.0),
    ("rows-63", "gauss", 63, 20, 3, (2, 3), 2, False, 1.0),
    ("rows-64-separable", "aligned", 64, 20, 3, (3,), 3, False, 1.0),
    ("rows-65-five-problems", "gauss", 65, 20, 10, (2, 3, 5, 4, 3), 4, False, 1.0),
    ("rows-511-duplicates", "duplicates", 511, 50, 2, (3,), 5, False, 1.0),
    ("rows-512-256-classes", "gauss", 512, 64, 2, (256,), 6, False, 1.0),
    ("rows-513-one-row-class", "single", 513, 50, 3, (2, 4), 7, False, 1.0),
    ("max-rows", "gauss", 16384, 100, 2, (2,), 8, False, 1.0),
    ("d17", "gauss", 300, 40, 17, (3,), 9, False, 1.0),
    ("d64-eight-problems", "gauss", 200, 40, 64, (2, 3, 2, 3, 2, 3, 2, 4), 10, False, 1.0),
    ("forty-classes-separable", "aligned", 1000, 100, 10, (40, 3), 11, False, 1.0),
    ("separable-257", "aligned", 257, 60, 2, (2, 3), 12, False, 1.0),
    ("offset-raw", "offset", 257, 43, 2, (2,), 13, False, 1.0),
    ("offset-scaled", "offset", 257, 43, 2, (2,), 13, True, 1.0),
    ("constant-zero-column", "constant", 130, 30, 3, (3,), 14, False, 1.0),
    ("constant-column-scaled", "constant", 130, 30, 3, (3,), 14, True, 1.0),
]
IDS = [c[0] for c in CASES]


def case(name):
    """The inputs and reference optima of a case (shared, unchanged: copy before writing)."""
    _n, family, S, T, D, classes, seed, scaled, reg_C = CASES[IDS.index(name)]
    got = dict(solved(family, S, T, D, classes, seed, scaled, reg_C))
    got.update(S=S, T=T, D=D, classes=list(classes), Q=len(classes), reg_C=reg_C, scaled=scaled)
    return got


# ---- InfoE --------------------------------------------------------------------------------------------------------------------------
def rank_labels(train, test, sizes):
    """(labels_train [K, S], labels_test [K, T] with -1 for a value the training rows do not hold, classes present per factor)."""
    lt, le, n = [], [], []
    stride = [int(np.prod(sizes[k + 1:])) for k in range(len(sizes))]
    for k, size in enumerate(sizes):
        vt, ve = (train // stride[k]) % size, (test // stride[k]) % size
        present = np.unique(vt)
        at = np.clip(np.searchsorted(present, ve), 0, len(present) - 1)
        lt.append(np.searchsorted(present, vt))
        le.append(np.where(present[at] == ve, at, -1))
        n.append(len(present))
    return np.stack(lt).astype(np.int32), np.stack(le).astype(np.int32), n


def infoe_reference(tab, sizes, train, test, reg_C=1.0, standardize=True, shift=None, scale=None):
    """infoe_from_table restated on the reference optimum (newton to 1e-13) -> its dictionary without the report."""
    tab = np.asarray(tab, dtype=np.float32)
    lt, le, n = rank_labels(train, test, sizes)
    if standardize and shift is None:
        shift, scale = standardizer(tab[train], len(train))
    Xt, Xe = features(tab[train], shift, scale), features(tab[test], shift, scale)
    K = len(sizes)
    out = {key: np.full(K, np.nan) for key in ("ce_model_train", "ce_model_test", "ce_null_train", "ce_null_test", "accuracy_train", "accuracy_test")}
    thetas = []
    for k, C in enumerate(n):
        theta, _its, gmax = newton(Xt, lt[k], C, reg_C)
        assert gmax <= 1e-13
        thetas.append(theta)
        freq = np.bincount(lt[k], minlength=C) / float(len(train))
        for name, X, lab in (("train", Xt, lt[k]), ("test", Xe, le[k])):
            got = predict(X, lab, theta, C)
            seen = lab >= 0
            with np.errstate(divide="ignore", invalid="ignore"):
                out["ce_model_" + name][k] = got["log_loss"] / got["counted"]
                out["ce_null_" + name][k] = -np.log(freq[lab[seen]]).sum() / got["counted"] if C > 1 else 0.0
            out["accuracy_" + name][k] = got["correct"] / float(len(lab))
    for name in ("train", "test"):
        out["infoe_%s_per_factor" % name], out["infoe_" + name] = infoe(out["ce_model_" + name], out["ce_null_" + name])
    out["thetas"], out["n_classes"], out["shift"], out["scale"] = thetas, n, shift, scale
    return out


def infoe(ce_model, ce_null):
    """1 - ce_model / ce_null per factor (NaN where ce_null is not positive), and the mean of max(0, .) over the others."""
    ce_model, ce_null = np.asarray(ce_model, dtype=np.float64), np.asarray(ce_null, dtype=np.float64)
    per = np.full(ce_model.shape, np.nan)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(ce_model) & (ce_null > 0)
    per[ok] = 1.0 - ce_model[ok] / ce_null[ok]
    return per, (float(np.maximum(per[ok], 0.0).mean()) if ok.any() else float("nan"))
