"""fp64 restatement (numpy, CPU) of the entropies and scores behind Evaluator.compute_separability_scores -- what the kernels of
csrc/latent_loo.hip and evaluate.separability_scores_from_entropies are judged by (a helper module, like decomp_ref.py) -- and
the tables the tests run them on.

S samples z_s = mu_n(s) + exp(logvar_n(s) / 2) eps_s, aggregate posterior q(z) = 1/N sum_n N(mu_n, diag exp(logvar_n)),
t_d(s, n) = log N(z_sd; mu_nd, exp(logvar_nd)):
    log q_!=i(z_s)  = logsumexp_n sum_{d != i} t_d(s, n) - log N          (D = 1: the empty sum, exactly 0)
    log q(z_s)      = logsumexp_n sum_d        t_d(s, n) - log N
    H_cond_d[i]     = 1/S sum_s 0.5 (log 2pi + logvar_n(s)i + eps_si^2)
"""
import math

import numpy as np

LOG2PI = math.log(2 * math.pi)
_TRIPLES = 1 << 21            # (sample, data point, dim) triples per temporary
GRIDS = ((8, 8, 4), (16, 16), (6, 5, 4, 3, 2))       # the grid tables of the tests: factor-aligned codes with sharp posteriors


def terms(z, mean, logvar, dtype=np.float64):
    """t_d(s, n) [S, N, D], every operation in `dtype`."""
    z, mean, logvar = (np.asarray(a, dtype=dtype) for a in (z, mean, logvar))
    half, c = dtype(0.5), dtype(LOG2PI)
    diff = z[:, None, :] - mean[None]
    return -half * (c + logvar[None]) - half * (diff * diff * np.exp(-logvar)[None])


def logsumexp(a, axis):
    """log sum exp over `axis` in fp64; a slice of -inf only gives -inf, never NaN."""
    a = np.asarray(a, dtype=np.float64)
    m = a.max(axis=axis, keepdims=True)
    shift = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return (np.log(np.exp(a - shift).sum(axis=axis, keepdims=True)) + shift).squeeze(axis)


def loo_sums(t):
    """[S, N, D] -> [D + 1, S, N]: row i < D the sum over d != i (np.delete-style: the other terms are ADDED), row D the sum over d."""
    D = t.shape[2]
    return np.stack([np.delete(t, i, axis=2).sum(axis=2) for i in range(D)] + [t.sum(axis=2)])


def loo_logq(z, mean, logvar):
    """-> log q_!=i(z_s) for i < D and log q(z_s) as row D: [D + 1, S] in fp64."""
    z, mean, logvar = (np.asarray(a, dtype=np.float64) for a in (z, mean, logvar))
    (S, D), N = z.shape, mean.shape[0]
    step = max(1, _TRIPLES // (N * D))
    out = [logsumexp(loo_sums(terms(z[s0:s0 + step], mean, logvar)), 2) - math.log(N) for s0 in range(0, S, step)]
    return np.concatenate(out, axis=1)


def cond_terms(eps, logvar, rows):
    """-> (H_cond_d [D], mean |term| [D]) in fp64."""
    eps, lv = np.asarray(eps, dtype=np.float64), np.asarray(logvar, dtype=np.float64)[np.asarray(rows)]
    term = 0.5 * (LOG2PI + lv + eps * eps)
    return term.mean(axis=0), np.abs(term).mean(axis=0)


def marginal_logq(z, mean, logvar):
    """-> log q_i(z_si) [D, S] in fp64."""
    z, mean, logvar = (np.asarray(a, dtype=np.float64) for a in (z, mean, logvar))
    (S, D), N = z.shape, mean.shape[0]
    step = max(1, _TRIPLES // (N * D))
    out = [logsumexp(terms(z[s0:s0 + step], mean, logvar), 1).T - math.log(N) for s0 in range(0, S, step)]
    return np.concatenate(out, axis=1)


def scores(H_z, H_z_d, H_loo, H_cond_d):
    """The combination of evaluate.separability_scores_from_entropies, restated with numpy."""
    H_z_d, H_loo, H_cond_d = (np.asarray(h, dtype=np.float64) for h in (H_z_d, H_loo, H_cond_d))
    D = len(H_z_d)
    info = H_z_d - H_cond_d
    mi = H_z - H_cond_d.sum()
    mi_loo = np.array([H_loo[i] - np.delete(H_cond_d, i).sum() for i in range(D)])
    sepin = mi - mi_loo
    w = np.maximum(info, 0.0)
    rho = w / w.sum() if w.sum() > 0 else np.zeros(D)
    ranked = np.sort(sepin)[::-1]
    return {"sepin": sepin, "wsepin": float((rho * sepin).sum()), "sepin_at_k": np.cumsum(ranked) / np.arange(1, D + 1),
            "informativeness": info, "redundancy": H_z_d + H_loo - H_z, "rho": rho, "mi": float(mi), "mi_loo": mi_loo,
            "dtc": float(H_loo.sum() - (D - 1) * H_z), "tc": float(H_z_d.sum() - H_z)}


def sample_z(mean, logvar, rows, eps):
    """fp32: the samples both sides are given."""
    mean, logvar, eps = (np.asarray(a, dtype=np.float32) for a in (mean, logvar, eps))
    return (mean[rows] + np.exp(np.float32(0.5) * logvar[rows]) * eps).astype(np.float32)


def evaluation(z, eps, rows, mean, logvar):
    """Every entropy and score of Evaluator.compute_separability_scores in fp64, plus the per-sample [D + 1, S] log-densities."""
    logq = loo_logq(z, mean, logvar)
    D = mean.shape[1]
    H = -logq.mean(axis=1)
    H_z_d = -marginal_logq(z, mean, logvar).mean(axis=1)
    H_cond_d, _ = cond_terms(eps, logvar, rows)
    out = scores(H[D], H_z_d, H[:D], H_cond_d)
    out.update(H_z=float(H[D]), H_z_d=H_z_d, H_loo=H[:D], H_cond_d=H_cond_d, logq=logq, n_samples=int(z.shape[0]), n_data=int(mean.shape[0]))
    return out


def derived_atol(ref):
    """decomp_ref.derived_atol extended by the new entropies: every score is a sum or difference of entropies that are each good
    to 1e-5 relative, so the sum of their magnitudes times 1e-5 bounds what cancellation leaves."""
    return 1e-5 * (np.abs(ref["H_z_d"]).sum() + abs(ref["H_z"]) + np.abs(ref["H_loo"]).sum() + np.abs(ref["H_cond_d"]).sum())


def grid_digits(sizes):
    """[N, D] digits of the row number in mixed radix `sizes` (the last dimension runs fastest)."""
    n = int(np.prod(sizes))
    return np.stack(np.unravel_index(np.arange(n), sizes), axis=1)


def grid_table(sizes, S, seed=0, jitter=0.05, product=False):
    """A factor-aligned code with sharp posteriors: N = prod(sizes) data points, D = len(sizes); means = 3.0 x the digits of the row
    number in mixed radix `sizes` plus jitter x sigma x N(0, 1); logvar uniform in [-10, -9.5]; S rows drawn without replacement.
    A data point that differs from a sample's own in ONE dimension has a term of about -1e5 there and is a dominant one of that
    dimension's leave-one-out density.  product=True: jitter 0 and a logvar that depends on (dimension, digit) alone -- every
    combination is present, so the aggregate posterior is the product of its marginals.
    -> mean, logvar [N, D] (fp32), rows [S] (int64), eps [S, D] (fp32)."""
    rng = np.random.RandomState(seed)
    digits = grid_digits(sizes)
    N, D = digits.shape
    if product:
        per_digit = [rng.uniform(-10.0, -9.5, size=k) for k in sizes]
        logvar = np.stack([per_digit[d][digits[:, d]] for d in range(D)], axis=1)
        jitter = 0.0
    else:
        logvar = rng.uniform(-10.0, -9.5, size=(N, D))
    mean = 3.0 * digits + jitter * np.exp(0.5 * logvar) * rng.standard_normal((N, D))
    rows = rng.permutation(N)[:S].astype(np.int64)
    eps = rng.standard_normal((S, D))
    return mean.astype(np.float32), logvar.astype(np.float32), rows, eps.astype(np.float32)


def fp32_loo_logq(z, mean, logvar, subtract):
    """The [D, S] leave-one-out log-densities with the terms and their sums over d in fp32 and the logsumexp in fp64.
    subtract=False: the other terms are added (prefix + suffix, as the kernel does); True: T - t_i, the form the kernel must
    never use."""
    t = terms(z, mean, logvar, dtype=np.float32)
    S, N, D = t.shape
    if subtract:
        total = np.zeros((S, N), dtype=np.float32)
        for d in range(D):
            total = total + t[:, :, d]
        sums = [total - t[:, :, i] for i in range(D)]
    else:
        sums = []
        for i in range(D):
            acc = None
            for d in [k for k in range(D) if k != i]:
                acc = t[:, :, d] if acc is None else acc + t[:, :, d]
            sums.append(acc)
    assert all(a.dtype == np.float32 for a in sums)
    return logsumexp(np.stack(sums), 2) - math.log(N)


def tolerance_multiple(got, ref):
    """max over samples of |got - ref| / (2e-6 |ref| + 2e-6): the project's per-sample tolerance, as a multiple."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    same = (got == ref)                                           # (-inf where the reference is -inf)
    with np.errstate(invalid="ignore"):
        m = np.abs(got - ref) / (2e-6 * np.abs(ref) + 2e-6)
    m = np.where(same, 0.0, m)
    return float(np.max(np.where(np.isnan(m), np.inf, m)))
