"""fp64 numpy restatement of the unsupervised disentanglement ranking (Duan et al. 2020; disentanglement_lib's udr.py) and of the
two statistics under it (a helper module, like unsup_ref.py): what Evaluator.compute_udr, udr_from_tables and the kernels of
csrc/latent_ranks.hip are judged by.  numpy only -- scipy and sklearn may be missing where the GPU tests run;
tests/test_udr_host.py compares this module with them where they exist.  Written from the definitions, independent of
disvae_amd/evaluate.py: ranks are a stable argsort plus searchsorted left and right, the Spearman correlation is numpy.corrcoef
of the ranks, the Lasso is coordinate descent on the Gram matrix of the standardised, masked representations.

The tolerance rules of tests/test_gpu_udr.py live here too, so that tests/test_udr_host.py can pin their precondition without a
GPU.  With u = 2^-53 and S selected rows:

  tol(kl[d])   = 8 S u m_d,  m_d = mean_s (mu^2 + e^lv + |lv| + 1) / 2: the project's accumulation bound form -- S u times the
                 mean magnitude of the terms, times the margin of 8 that unsup_ref.cov_tolerance carries.
  tol(R[a, b]) = tc / sqrt(va vb) + |c| / sqrt(va vb) (tva / (2 va) + tvb / (2 vb)): first-order propagation, through
                 c / sqrt(va vb), of unsup_ref.cov_tolerance (the bound documented for dvae_unsup_moments) of the table the
                 correlation is taken of -- tc, tva, tvb its entries for the covariance and the two variances.  No new constant.
  tol(score)   = max tol(R) (D + 2) / 0.1: a pair score is a mean of terms max^2 / sum over the rows and columns of R.  One term
                 moves by (2 max / sum) d max - (max / sum)^2 d sum with |d max| <= tol(R), |d sum| <= D tol(R) and max <= sum:
                 (D + 2) tol(R) to first order; the division by 0.1 -- the least row or column sum, pinned on the CPU for the
                 end-to-end cases -- covers what lies beyond first order in d sum / sum.
  tol(|w|)     = max(1, |G_AA^-1|) ((1 + |w|_1) max tol(G) + 2e-13 |G|)  (norms: infinity) for the Lasso coefficients of one
                 output: on the active set A the optimum solves G_AA w_A = c_A - alpha sign(w_A), so d w_A = G_AA^-1 (d c - d G w);
                 an inactive coefficient moves by at most the same d c - d G w when it crosses the threshold (the max(1, .));
                 both descents stop at a sweep that moves w by at most 1e-13, which leaves a residual of at most |G| 1e-13 each.
"""
import functools

import numpy as np

import info_ref as I
import unsup_ref as UR

U = 2.0 ** -53


# ---- ranks ----------------------------------------------------------------------------------------------------------------------
def ranks(table, rows=None):
    """fp64 [S, D]: the 1-based tie-averaged rank of every element within its column (scipy.stats.rankdata(method="average")):
    #{smaller} + (#{equal} + 1) / 2 by searchsorted left and right on the sorted column; x + 0.0 folds -0 into +0."""
    x = UR.select(table, rows)
    out = np.empty(x.shape, dtype=np.float64)
    for d in range(x.shape[1]):
        col = x[:, d] + np.float32(0.0)
        srt = col[np.argsort(col, kind="stable")]
        lo, hi = np.searchsorted(srt, col, side="left"), np.searchsorted(srt, col, side="right")
        out[:, d] = lo + (hi - lo + 1) / 2.0
    return out


# ---- KL -------------------------------------------------------------------------------------------------------------------------
def kl_dims(mean, logvar, rows=None):
    mu, lv = UR.select(mean, rows).astype(np.float64), UR.select(logvar, rows).astype(np.float64)
    return (0.5 * (mu * mu + np.exp(lv) - lv - 1.0)).mean(axis=0)


def kl_tolerance(mean, logvar, rows=None):
    mu, lv = UR.select(mean, rows).astype(np.float64), UR.select(logvar, rows).astype(np.float64)
    return 8 * mu.shape[0] * U * (0.5 * (mu * mu + np.exp(lv) + np.abs(lv) + 1.0)).mean(axis=0)


# ---- correlations ---------------------------------------------------------------------------------------------------------------
def _corr(x, y):
    """|Pearson correlation| [Dx, Dy] of the columns of x with those of y, fp64, 0 where a column is constant"""
    xc, yc = x - x.mean(axis=0), y - y.mean(axis=0)
    sx, sy = np.sqrt((xc * xc).sum(axis=0)), np.sqrt((yc * yc).sum(axis=0))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = (xc.T @ yc) / np.outer(sx, sy)
    r[~np.isfinite(r)] = 0.0
    r[sx == 0, :] = 0.0
    r[:, sy == 0] = 0.0
    return np.abs(r)


def spearman(mean_a, mean_b, mask_a, mask_b, rows=None):
    r = _corr(ranks(mean_a, rows), ranks(mean_b, rows))
    r[~mask_a, :] = 0.0
    r[:, ~mask_b] = 0.0
    return r


def standardised(mean, mask, rows=None):
    """disentanglement_lib's representation of one model: StandardScaler (ddof = 0; a constant column becomes 0), then the
    uninformative latents zeroed"""
    x = UR.select(mean, rows).astype(np.float64)
    xc = x - x.mean(axis=0)
    s = np.sqrt((xc * xc).mean(axis=0))
    z = np.divide(xc, s, out=np.zeros_like(xc), where=s > 0)
    z[:, s == 0] = 0.0
    return z * mask


def lasso_gram(G, c, alpha, stop=1e-13, max_sweeps=100000):
    """cyclic coordinate descent for (1 / 2S) ||y - X w||^2 + alpha ||w||_1 from G = X^T X / S and c = X^T y / S"""
    w = np.zeros(len(c))
    for _ in range(max_sweeps):
        worst = 0.0
        for a in range(len(c)):
            if G[a, a] == 0:
                continue
            rho = c[a] - (G[a] @ w - G[a, a] * w[a])
            new = np.sign(rho) * max(abs(rho) - alpha, 0.0) / G[a, a]
            worst, w[a] = max(worst, abs(new - w[a])), new
        if worst <= stop:
            break
    return w


def lasso(mean_a, mean_b, mask_a, mask_b, alpha=0.1, rows=None):
    x, y = standardised(mean_a, mask_a, rows), standardised(mean_b, mask_b, rows)
    S = x.shape[0]
    G, C = x.T @ x / S, x.T @ y / S
    return np.stack([np.abs(lasso_gram(G, C[:, b], alpha)) for b in range(y.shape[1])], axis=1)


# ---- scores ---------------------------------------------------------------------------------------------------------------------
def pair_score(R):
    R = np.asarray(R, dtype=np.float64)
    if R.size == 0:
        return 0.0
    out = 0.0
    for axis in (0, 1):
        top, total = R.max(axis=axis) ** 2, R.sum(axis=axis)
        out += 0.5 * np.mean([t / s if s > 0 else 0.0 for t, s in zip(top, total)])
    return float(out)


def model_scores(pairwise):
    M = pairwise.shape[0]
    return np.array([np.median([pairwise[j, i] for j in range(M) if j != i]) for i in range(M)])


def udr(means, logvars, correlation="spearman", rows=None, kl_threshold=0.01, filter_low_kl=True, lasso_alpha=0.1):
    M, D = len(means), means[0].shape[1]
    kl = np.stack([kl_dims(m, lv, rows) for m, lv in zip(means, logvars)])
    mask = kl > kl_threshold
    raw, pairwise = np.zeros((M, M, D, D)), np.zeros((M, M))
    for i in range(M):
        for j in range(M):
            if i == j:
                continue
            if correlation == "spearman":
                raw[i, j] = spearman(means[i], means[j], mask[i], mask[j], rows)
            else:
                raw[i, j] = lasso(means[i], means[j], mask[i], mask[j], lasso_alpha, rows)
            R = raw[i, j][np.ix_(mask[i], mask[j])] if filter_low_kl else raw[i, j]
            pairwise[i, j] = pair_score(R)
    return {"model_scores": model_scores(pairwise), "pairwise_scores": pairwise, "raw_correlations": raw, "kl": kl,
            "n_active": mask.sum(axis=1), "n_samples": UR.select(means[0], rows).shape[0], "correlation": correlation}


# ---- tolerances -----------------------------------------------------------------------------------------------------------------
def correlation_tolerance(x, y):
    """tol(R) [Dx, Dy] of the module docstring for the correlation of the columns of x with those of y (fp64 [S, D] tables: the
    ranks, or the raw means); inf where a variance is 0 (R is then an exact 0 on both sides and is compared as such)"""
    both = np.concatenate([x, y], axis=1).astype(np.float32)
    mom = UR.moments(both)
    tol, cov, D = UR.cov_tolerance(mom), mom["cov"], x.shape[1]
    v, tv = np.diag(cov), np.diag(tol)
    with np.errstate(divide="ignore", invalid="ignore"):
        root = np.sqrt(np.outer(v[:D], v[D:]))
        out = tol[:D, D:] / root + np.abs(cov[:D, D:]) / root * (tv[:D, None] / (2 * v[:D, None]) + tv[None, D:] / (2 * v[None, D:]))
    out[~np.isfinite(out)] = 0.0
    return out


def gram_tolerance(x):
    return correlation_tolerance(x, x)


def lasso_tolerance(mean_a, mean_b, mask_a, mask_b, alpha=0.1, rows=None):
    """tol(|w|) [D, D] of the module docstring, one value per output latent (column)"""
    x, y = standardised(mean_a, mask_a, rows), standardised(mean_b, mask_b, rows)
    S, D = x.shape
    G, W = x.T @ x / S, lasso(mean_a, mean_b, mask_a, mask_b, alpha, rows)
    raw_a, raw_b = select(mean_a, rows).astype(np.float64), select(mean_b, rows).astype(np.float64)
    t = max(gram_tolerance(raw_a).max(), correlation_tolerance(raw_a, raw_b).max())
    out = np.zeros((D, D))
    for b in range(D):
        act = W[:, b] != 0
        inv = np.abs(np.linalg.inv(G[np.ix_(act, act)])).sum(axis=1).max() if act.any() else 0.0
        out[:, b] = max(1.0, inv) * ((1 + W[:, b].sum()) * t + 2e-13 * np.abs(G).sum(axis=1).max())
    return out


def select(table, rows=None):
    return UR.select(table, rows)


def score_tolerance(tol_R, D):
    return float(np.max(tol_R)) * (D + 2) / 0.1


# ---- tables ---------------------------------------------------------------------------------------------------------------------
def _f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def _bits(u):
    return np.asarray(u, dtype=np.uint32).view(np.float32)


def hard_table(kind, S, D=3):
    """fp32 [S, D] tables built to break a radix sort.  const / ties / gauss are info_ref.make_table's (what tests/irs_ref.py
    generates its cases from); the others are made here."""
    rng = np.random.default_rng(S * 131 + D)
    if kind in ("const", "ties", "gauss"):
        return I.make_table((S,), D, kind)
    if kind == "two":                                                        # two alternating values
        return _f32(np.where((np.arange(S)[:, None] + np.arange(D)) % 2 == 0, 1.5, -0.25))
    if kind == "quarters":                                                   # runs that straddle chunk edges
        return _f32(np.round(rng.standard_normal((S, D)) * 4) / 4)
    if kind == "sorted":
        return _f32(np.sort(rng.standard_normal((S, D)), axis=0))
    if kind == "reversed":
        return _f32(np.sort(rng.standard_normal((S, D)), axis=0)[::-1])
    if kind == "zeros":                                                      # +0, -0 and their neighbours
        return _f32(rng.choice(np.array([0.0, -0.0, 1e-45, -1e-45, 1.0, -1.0], dtype=np.float32), size=(S, D)))
    if kind == "negative":
        return _f32(-np.abs(rng.standard_normal((S, D))) - 1e-3)
    if kind == "low_byte":                                                   # keys that differ in the lowest mantissa byte only
        return _bits(0x3F800000 + rng.integers(0, 256, size=(S, D)))
    if kind == "exponent":                                                   # ... in the exponent only
        return _bits((rng.integers(1, 255, size=(S, D)) << 23) | 0x00400000)
    if kind == "sign":                                                       # ... in the sign only
        return _bits((rng.integers(0, 2, size=(S, D)) << 31) | 0x3FC00000)
    if kind == "denormal":
        return _bits((rng.integers(0, 2, size=(S, D)) << 31) | rng.integers(0, 1 << 12, size=(S, D)))
    raise ValueError(kind)


HARD = ("const", "ties", "two", "quarters", "sorted", "reversed", "zeros", "negative", "low_byte", "exponent", "sign", "denormal")


def size_cases(lib):
    """(S, D): S in 1, 2, 63, 64, 65, one tile (256 keys) +- 1; every D of 1, 3, 10, 64; three chunks with a short last one"""
    three = 2 * lib.CHUNK_ROWS + 4                                           # 3 chunks of 1367, the last one 1366
    assert three > lib.SMALL_ROWS and -(-three // lib.CHUNK_ROWS) == 3 and three % 3 != 0
    return [(1, 3), (2, 1), (63, 10), (64, 3), (65, 64), (255, 3), (256, 10), (257, 1), (three, 3), (three, 64)]


def switch_cases(lib):
    """(S, D): the last shape below and the first above every dispatch macro of include/dvae_udr_hip.h for the ranks
    (lib = disvae_amd._udrlib, which mirrors them); the chunk-growth cap with D = 1"""
    assert lib.SMALL_ROWS >= lib.CHUNK_ROWS                                  # above SMALL_ROWS there are two chunks or more
    cap = lib.CHUNK_ROWS * lib.MAX_CHUNKS
    return [(lib.SMALL_ROWS, 3), (lib.SMALL_ROWS + 1, 3), (cap, 1), (cap + 1, 1)]


def kl_switch_cases(lib):
    """S: one chunk / two of the KL pass, and its cap"""
    cap = lib.KL_BLOCK_ROWS * lib.KL_MAX_CHUNKS
    return [lib.KL_BLOCK_ROWS, lib.KL_BLOCK_ROWS + 1, cap, cap + 1]


@functools.lru_cache(maxsize=None)
def rank_case(kind, S, D):
    """table and its reference ranks (fp32: every half-integer up to 2^23 is one): computed once, shared, never modified"""
    table = hard_table(kind, S, D)
    return table, ranks(table).astype(np.float32)


# ---- end to end -----------------------------------------------------------------------------------------------------------------
def _warp(z, k):
    """a strictly increasing function, another one for every k"""
    return (z + 0.3 * z ** 3, np.sinh(z), 2 * z + 1)[k % 3]


@functools.lru_cache(maxsize=None)
def sweep(kind, D, S=2000, M=3):
    """M models as (means, logvars), fp32 [S, D] each.  "aligned": signed, permuted, monotonically warped copies of one Gaussian
    table plus 2 % noise -- the same factors axis by axis; "rotated": as aligned, but model 1 mixes its latents pairwise by 45
    degrees; "collapsed": aligned with every latent of model 2 under the KL threshold (mean 1e-3 noise, logvar 0).  The last
    latent of every model (D >= 3) is collapsed throughout."""
    rng = np.random.default_rng(7 + D)
    z = rng.standard_normal((S, D))
    means, logvars = [], []
    for m in range(M):
        live = D - 1 if D >= 3 else D                                        # every model keeps the SAME factors: the last one is dropped
        perm, sign = np.concatenate([rng.permutation(live), np.arange(live, D)]), rng.choice([-1.0, 1.0], size=D)
        x = np.stack([sign[d] * _warp(z[:, perm[d]], m + d) for d in range(D)], axis=1) + 0.02 * rng.standard_normal((S, D))
        if kind == "rotated" and m == 1:
            for d in range(0, live - 1, 2):
                a, b = x[:, d] / x[:, d].std(), x[:, d + 1] / x[:, d + 1].std()
                x[:, d], x[:, d + 1] = (a + b) / np.sqrt(2.0), (a - b) / np.sqrt(2.0)
        lv = -6.0 + 0.3 * rng.standard_normal((S, D))
        if D >= 3 or (kind == "collapsed" and m == 2):
            dead = slice(None) if (kind == "collapsed" and m == 2) else slice(D - 1, D)
            x[:, dead] = 1e-3 * rng.standard_normal(x[:, dead].shape)
            lv[:, dead] = 0.01 * rng.standard_normal(lv[:, dead].shape)
        means.append(_f32(x))
        logvars.append(_f32(lv))
    return tuple(means), tuple(logvars)


END_TO_END = [("aligned", 2), ("aligned", 10), ("rotated", 2), ("rotated", 10)]
