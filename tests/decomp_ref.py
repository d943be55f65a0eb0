"""fp64 restatement (plain torch, CPU) of the data-set level ELBO decomposition of Chen et al. 2018, section 3 -- what
Evaluator.compute_elbo_decomposition and the kernels of csrc/elbo_decomp.hip are judged by (a helper module, like gpu_util.py).

S samples z_s = mu_n(s) + exp(logvar_n(s) / 2) eps_s, aggregate posterior q(z) = 1/N sum_n N(mu_n, diag exp(logvar_n)):
    log q(z_s)          = logsumexp_n sum_d log N(z_sd; mu_nd, exp(logvar_nd)) - log N
    log q_d(z_sd)       = logsumexp_n       log N(z_sd; mu_nd, exp(logvar_nd)) - log N
    log q(z_s | x_n(s)) = sum_d [-0.5 (log 2pi + logvar_n(s)d) - 0.5 eps_sd^2]
    log p(z_s)          = sum_d [-0.5 log 2pi - 0.5 z_sd^2]
"""
import math

import torch

LOG2PI = math.log(2 * math.pi)
_PAIRS = 1 << 21            # (sample, data point, dim) triples per temporary


def log_density(z, mu, logvar):
    """log N(z; mu, exp(logvar)), the reference's log_density_gaussian (utils/math.py:48-50)."""
    return -0.5 * (LOG2PI + logvar) - 0.5 * (z - mu) ** 2 * torch.exp(-logvar)


def aggregate_logq(z, mean, logvar):
    """-> (log q(z_s) [S], log q_d(z_sd) [S, D]) in fp64."""
    z, mean, logvar = z.double(), mean.double(), logvar.double()
    (S, D), N = z.shape, mean.shape[0]
    step = max(1, _PAIRS // (N * D))
    joint, marg = [], []
    for s0 in range(0, S, step):
        ld = log_density(z[s0:s0 + step, None, :], mean[None], logvar[None])            # [s, N, D]
        joint.append(torch.logsumexp(ld.sum(2), 1) - math.log(N))
        marg.append(torch.logsumexp(ld, 1) - math.log(N))
    return torch.cat(joint), torch.cat(marg)


def sample_terms(z, eps, logvar, rows):
    """-> (log q(z_s | x_n(s)) [S], log p(z_s) [S]) in fp64."""
    z, eps, lv = z.double(), eps.double(), logvar.double().index_select(0, rows)
    return (-0.5 * (LOG2PI + lv) - 0.5 * eps ** 2).sum(1), (-0.5 * LOG2PI - 0.5 * z ** 2).sum(1)


def sample_z(mean, logvar, rows, eps):
    return mean.index_select(0, rows) + torch.exp(0.5 * logvar.index_select(0, rows)) * eps


def decomposition(z, eps, rows, mean, logvar):
    """The dict of Evaluator.compute_elbo_decomposition (python floats, fp64 arithmetic) plus the per-sample tensors."""
    logqz, logqz_d = aggregate_logq(z, mean, logvar)
    logqz_condx, logpz = sample_terms(z, eps, logvar, rows)
    H_z, H_z_d, H_zCx = -logqz.mean().item(), [-v.item() for v in logqz_d.mean(0)], -logqz_condx.mean().item()
    mean_logpz = logpz.mean().item()
    mi = H_z - H_zCx
    tc = math.fsum(H_z_d) - H_z
    dw_kl = -math.fsum(H_z_d) - mean_logpz
    return {"H_z": H_z, "H_z_d": H_z_d, "H_zCx": H_zCx, "mi": mi, "tc": tc, "dw_kl": dw_kl, "kl": mi + tc + dw_kl,
            "n_samples": int(z.shape[0]), "n_data": int(mean.shape[0]),
            "mean_logpz": mean_logpz, "logqz": logqz, "logqz_condx": logqz_condx, "logpz": logpz}


def derived_atol(ref):
    """mi, tc, dw_kl and kl are differences of the entropies and means, each good to 1e-5 relative: the sum of their magnitudes
    times 1e-5 bounds what cancellation leaves."""
    return 1e-5 * (sum(abs(h) for h in ref["H_z_d"]) + abs(ref["H_z"]) + abs(ref["H_zCx"]) + abs(ref["mean_logpz"]))


def clustered_posteriors(N, D, S, seed, logvar_range=(-2.0, 0.5)):
    """Posteriors whose aggregate is a real mixture: means = 0.3 randn + one of 8 cluster offsets, logvar uniform in the range.
    (Unclustered random means in many dimensions saturate I[z;n] at log N: every sample then sees its own row only.)
    -> mean, logvar [N, D], rows [S] (distinct while S <= N, else drawn with replacement: the kernels take any rows), eps [S, D]."""
    gen = torch.Generator().manual_seed(seed)
    centers = 2.0 * torch.randn(8, D, generator=gen)
    mean = 0.3 * torch.randn(N, D, generator=gen) + centers[torch.arange(N) % 8]
    lo, hi = logvar_range
    logvar = lo + (hi - lo) * torch.rand(N, D, generator=gen)
    rows = torch.randperm(N, generator=gen)[:S] if S <= N else torch.randint(0, N, (S,), generator=gen)
    eps = torch.randn(S, D, generator=gen)
    return mean, logvar, rows.contiguous(), eps
