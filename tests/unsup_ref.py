"""fp64 numpy restatement of the label-free scores (disentanglement_lib's unsupervised_metrics.py: Gaussian total correlation,
Gaussian Wasserstein correlation, mean pairwise mutual information of the discretised latents) and of the two statistics under
them (a helper module, like info_ref.py): what Evaluator.compute_unsupervised_scores and the kernels of csrc/latent_pairs.hip are
judged by.  Written from the definitions, independent of disvae_amd/evaluate.py: moments are numpy.cov(ddof=1) in fp64, binning
is numpy.histogram + numpy.digitize literally, the pair counts are numpy.add.at, the mutual information is
info_ref.mutual_information.  The tables are those of info_ref.make_table; their lat_sizes serve as row counts only.

The tolerance rules of tests/test_gpu_unsupervised_scores.py live here too, so that tests/test_unsupervised_scores_host.py can
pin their precondition without a GPU.  With u = 2^-53, S selected rows and m2_d the fp64 mean of (x_d - x0_d)^2 (x0: the first
selected row, which the kernel shifts by):

  tol(cov[d, e]) = 8 S u sqrt(m2_d m2_e)
  tol(mean[d])   = 8 S u sqrt(m2_d) + u |mean_d|

the worst-case rounding of an S-term fp64 sum -- S u times the sum of the terms' magnitudes, which is at most S sqrt(m2_d m2_e)
by Cauchy-Schwarz, divided by S - 1 >= S / 2 -- times a margin of 4 for the two sums (of products and plain) and the final
combination: 5e-14 relative at S = 60 and 6.5e-10 at S = 737 280.  An fp32 accumulation misses it by orders of magnitude at every
S used.

  tol(score) = 2 D cond(R) max_de tol(cov[d, e]) / sqrt(v_d v_e)   for the total correlation and both Wasserstein scores, R the
                                                 fp64 correlation matrix of the live block, v its variances: first-order
                                                 perturbation of logdet (|d logdet| <= D ||R^-1|| ||dR||) and of the eigenvalues;
                                                 the 2 is the only margin.
"""
import functools

import numpy as np

import info_ref as I

U = 2.0 ** -53


# ---- tables ---------------------------------------------------------------------------------------------------------------------
def make_table(lat_sizes, D, family):
    """info_ref.make_table, and "mixed": its gauss table with every third column collapsed -- columns 1, 4, 7, ... exactly constant
    (every row in ONE bin), column 2 (where there is one) at std 0.05 around a constant: live, but no active unit -- beside the live
    ones.  (Not smaller: the restatement takes the Wasserstein correlation from numpy.linalg.eigvalsh of V^1/2 C V^1/2, whose small
    eigenvalues carry an ABSOLUTE error of 2^-53 max(v)^2; below a variance of about 1e-4 max(v) the square root of that passes the
    bound of the Gaussian scores.  The same holds for evaluate.py, which says so.)"""
    if family != "mixed":
        return I.make_table(lat_sizes, D, family)
    t = I.make_table(lat_sizes, D, "gauss").astype(np.float64)
    t[:, 1::3] = 0.3
    if D > 2:
        t[:, 2] = -1.5 + 0.05 * (t[:, 2] - t[:, 2].mean()) / t[:, 2].std()
    return np.ascontiguousarray(t.astype(np.float32))


def select(table, rows=None):
    return table if rows is None else table[rows]


# ---- statistics -----------------------------------------------------------------------------------------------------------------
def moments(table, rows=None):
    """min, max (the fp32 elements), fp64 mean [D] and numpy.cov(ddof=1) [D, D] (zeros when one row is selected), and m2 [D], the
    fp64 mean of (x - x0)^2 that the tolerances are made of."""
    x = select(table, rows)
    S, D = x.shape
    x64 = x.astype(np.float64)
    cov = np.atleast_2d(np.cov(x64.T, ddof=1)) if S > 1 else np.zeros((D, D))
    return {"min": x.min(axis=0), "max": x.max(axis=0), "mean": x64.mean(axis=0), "cov": cov,
            "m2": ((x64 - x64[0]) ** 2).mean(axis=0), "S": S}


def cov_tolerance(mom):
    return 8 * mom["S"] * U * np.sqrt(mom["m2"][:, None] * mom["m2"][None, :])


def mean_tolerance(mom):
    return 8 * mom["S"] * U * np.sqrt(mom["m2"]) + U * np.abs(mom["mean"])


def chunked_moments(table, rows=None, chunk=1024):
    """the first-row-shifted sums as a device would take them: fp64, chunks of `chunk` rows each summed on its own, the chunks added
    in order -> (mean [D], cov [D, D])"""
    x = select(table, rows).astype(np.float64)
    S, D = x.shape
    dx = x - x[0]
    s1, s2 = np.zeros(D), np.zeros((D, D))
    for c in range(0, S, chunk):
        part = dx[c:c + chunk]
        s1 += part.sum(axis=0)
        s2 += part.T @ part
    cov = (s2 - np.outer(s1, s1) / S) / (S - 1) if S > 1 else np.zeros((D, D))
    return x[0] + s1 / S, cov


def pair_list(D):
    """(d, e), d < e, in lexicographic order: the pairs of dvae_unsup_pair_hist"""
    return [(d, e) for d in range(D) for e in range(d + 1, D)]


def pair_counts(table, n_bins, rows=None):
    """-> (counts int64 [D (D - 1) / 2, n_bins, n_bins], edges fp32 [D, n_bins]): numpy.histogram's edges per selected column,
    numpy.digitize, numpy.add.at."""
    x = select(table, rows)
    S, D = x.shape
    edges = np.stack([I.lower_edges(x[:, d], n_bins) for d in range(D)])
    bins = np.stack([I.bins_of(x[:, d], edges[d]) for d in range(D)])                       # [D, S]
    pairs = pair_list(D)
    counts = np.zeros((len(pairs), n_bins, n_bins), dtype=np.int64)
    if pairs:
        d, e = (np.array(c) for c in zip(*pairs))
        p = np.broadcast_to(np.arange(len(pairs))[:, None], (len(pairs), S))
        np.add.at(counts, (p, bins[d], bins[e]), 1)
    return counts, edges


# ---- scores ---------------------------------------------------------------------------------------------------------------------
def gaussian_scores(cov, live):
    """(total correlation, Wasserstein correlation, normalised) of the covariance restricted to the live columns"""
    C = cov[np.ix_(live, live)]
    v = np.diag(C)
    tc = wass = norm = 0.0
    if live.sum() >= 2:
        sign, logdet = np.linalg.slogdet(C)
        tc = 0.5 * (np.sum(np.log(v)) - logdet) if sign > 0 else np.inf
    if live.sum() >= 1:
        half = np.diag(np.sqrt(v))
        lam = np.linalg.eigvalsh(half @ C @ half)
        wass = 2 * np.trace(C) - 2 * np.sqrt(lam.clip(min=0)).sum()
        norm = wass / np.sum(v)
    return float(tc), float(wass), float(norm)


def scores(table, n_bins=20, rows=None, active_threshold=0.01):
    mom = moments(table, rows)
    D = table.shape[1]
    live = mom["max"] > mom["min"]
    tc, wass, norm = gaussian_scores(mom["cov"], live)
    counts, _ = pair_counts(table, n_bins, rows)
    mi = np.zeros((D, D))
    for p, (d, e) in enumerate(pair_list(D)):
        mi[d, e] = mi[e, d] = I.mutual_information(counts[p])
    return {"gaussian_total_correlation": tc, "gaussian_wasserstein_correlation": wass, "gaussian_wasserstein_correlation_norm": norm,
            "mutual_info_score": float(mi.sum() / (D * D - D)) if D > 1 else 0.0, "mutual_information": mi,
            "active_units": int((np.diag(mom["cov"]) > active_threshold).sum()), "variances": np.diag(mom["cov"]).copy(), "live": live,
            "n_samples": mom["S"], "n_bins": n_bins}


def live_correlation(mom):
    live = mom["max"] > mom["min"]
    C = mom["cov"][np.ix_(live, live)]
    s = np.sqrt(np.diag(C))
    return C / np.outer(s, s), live


def score_tolerance(mom):
    """the bound of the three Gaussian scores (module docstring); 0 without a live column: the scores are then exact zeros"""
    R, live = live_correlation(mom)
    if not live.any():
        return 0.0
    v = np.diag(mom["cov"])[live]
    rel = cov_tolerance(mom)[np.ix_(live, live)] / np.sqrt(np.outer(v, v))
    return float(2 * mom["cov"].shape[0] * np.linalg.cond(R) * rel.max())


def worst_ratio(got, ref, tol):
    return I.worst_ratio(got, ref, tol)


# ---- the shapes of tests/test_gpu_unsupervised_scores.py ------------------------------------------------------------------------
_L = [(60,), (3, 4, 5), (2, 3, 6, 40)]                       # 60, 60 and 1440 rows
# (lat_sizes, D, n_bins, family, S): every D of {1, 2, 3, 10, 17, 64}, every n_bins of {1, 2, 7, 20, 64}, every family, every
# selection of {None, 1, 63, 65, 10000}; S: that many rows drawn with repeats.  D = 1 has no pair: moments only.
CASES = [(_L[0], 1, 20, "gauss", None), (_L[0], 2, 1, "gauss", None), (_L[0], 64, 64, "ties", None), (_L[0], 3, 2, "disent", 65),
         (_L[1], 3, 20, "ties", None), (_L[1], 17, 7, "gauss", 63), (_L[1], 10, 20, "const", None), (_L[1], 2, 64, "offset", 65),
         (_L[1], 1, 7, "offset", 10000), (_L[1], 10, 20, "mixed", 1),
         (_L[2], 10, 20, "disent", None), (_L[2], 64, 2, "gauss", None), (_L[2], 3, 20, "offset", 10000),
         (_L[2], 10, 20, "mixed", 10000), (_L[2], 17, 20, "gauss", 1), (_L[2], 10, 7, "mixed", None), (_L[2], 2, 64, "ties", 63)]
# (family or "ideal" / "rotated" is not used here: the Gaussian scores need a well-conditioned live block) (lat, D, n_bins, S)
END_TO_END = [("gauss", _L[1], 3, 20, None), ("offset", _L[2], 10, 20, None), ("ties", _L[0], 17, 7, None), ("const", _L[1], 4, 20, None),
              ("disent", _L[2], 4, 20, None), ("mixed", _L[2], 10, 20, None), ("gauss", _L[2], 10, 64, 65), ("offset", _L[2], 3, 2, 10000),
              ("mixed", _L[1], 10, 20, 1), ("gauss", _L[0], 1, 20, None), ("gauss", _L[1], 2, 1, None)]


def tile_dims(lib, n_bins=20):
    """(the last D whose pairs fit one LDS tile at n_bins, the first that needs two)"""
    per_tile = max(lib.HIST_LDS_INTS // (n_bins * n_bins), 1)
    D = 2
    while (D + 1) * D // 2 <= per_tile:
        D += 1
    return D, D + 1


def switch_cases(lib):
    """(lat_sizes, D, n_bins, family, S): the last shape below and the first above every dispatch macro of
    include/dvae_unsup_hip.h (lib = disvae_amd._unsuplib, which mirrors them).  Large S on a 60-row table: the rows repeat, the
    table stays small."""
    out = []
    for rows in (lib.MOMENTS_BLOCK_ROWS, lib.HIST_BLOCK_ROWS):                               # one workgroup / two
        out += [(_L[1], 3, 20, "offset", rows), (_L[1], 3, 20, "offset", rows + 1)]
    for rows in (lib.MOMENTS_BLOCK_ROWS * lib.MAX_BLOCKS, lib.HIST_BLOCK_ROWS * lib.MAX_BLOCKS):   # the grid stops growing
        out += [(_L[0], 2, 20, "gauss", rows), (_L[0], 2, 20, "gauss", rows + 1)]
    one, two = tile_dims(lib)                                                                # one tile of pairs / two
    out += [(_L[1], one, 20, "gauss", None), (_L[1], two, 20, "gauss", None)]
    assert lib.HIST_LDS_INTS // lib.MAX_BINS ** 2 == 1                                       # the most bins: one pair per tile
    out += [(_L[1], 3, lib.MAX_BINS, "gauss", None)]
    D = 1                                                                                    # a second sum per thread of the moments pass
    while (D + 1) * (D + 4) // 2 <= 256:
        D += 1
    assert D * (D + 3) // 2 <= 256 < (D + 1) * (D + 4) // 2 and lib.MOMENTS_THREAD_SUMS * 256 >= lib.MAX_D * (lib.MAX_D + 3) // 2
    out += [(_L[2], D, 2, "gauss", None), (_L[2], D + 1, 2, "gauss", None)]
    return out


@functools.lru_cache(maxsize=None)
def case(lat_sizes, D, n_bins, family, S):
    """Table, rows (None: all; else S random rows with repeats) and the fp64 statistics: computed once, shared, never modified."""
    table = make_table(lat_sizes, D, family)
    rows = None
    if S is not None:
        rows = np.random.default_rng(S + D).integers(0, table.shape[0], size=S)
    counts, edges = pair_counts(table, n_bins, rows)
    return {"table": table, "rows": rows, "counts": counts, "edges": edges, "moments": moments(table, rows)}


def end_to_end_case(kind, lat_sizes, D, n_bins, S):
    table = make_table(lat_sizes, D, kind)
    rows = None if S is None else np.random.default_rng(S + D).integers(0, table.shape[0], size=S)
    return table, rows
