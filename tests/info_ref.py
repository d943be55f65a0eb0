"""fp64 numpy restatement of the discretised MIG, modularity and continuous-factor SAP scores and of the two statistics under
them (a helper module, like scores_ref.py): what Evaluator.compute_information_scores and the kernels of csrc/factor_info.hip
are judged by.  Written from the definitions -- disentanglement_lib's mig.py, modularity_explicitness.py, sap_score.py --
independent of disvae_amd/evaluate.py: binning is numpy.histogram + numpy.digitize literally, moments are numpy.cov(ddof=1) in
fp64, the factor values are materialised with numpy.indices.

The tolerance rule of tests/test_gpu_information_scores.py lives here too, so that tests/test_information_scores_host.py can pin
its precondition without a GPU (the rule of tests/latent_regimes.py):

  tol of a covariance of columns i, j:  1e-5 s_i s_j + 4 * 2^-24 (a_i s_j + a_j s_i) / 2,  s = sqrt(fp64 variance), a = max |x|
                                        (i = j: the variance tolerance of tests/test_gpu_factor_scores.py);
  tol of a mean:                        1e-5 s + 4 * 2^-24 a  (the rounding of the fp32 result is 2^-24 a at most);
  e32 = worst |fp32 restatement - fp64| / tol, the fp32 restatement being the same centred sums (shift by the first row, mean,
  deviations) with numpy's pairwise fp32 sums; a kernel passes at ratio <= max(1, 4 e32); e32 > CAP = 2.5 is a wrong INPUT.
"""
import functools

import numpy as np

CAP = 2.5
MARGIN = 4.0


def bound(e32):
    return max(1.0, MARGIN * e32)


# ---- the data set ---------------------------------------------------------------------------------------------------------------
def factor_values(lat_sizes):
    """int64 [N, K]: the value index of every factor for every row of a data set that enumerates lat_sizes in row-major order."""
    return np.indices(tuple(int(s) for s in lat_sizes)).reshape(len(lat_sizes), -1).T.astype(np.int64)


def select(table, lat_sizes, rows=None):
    """-> (x fp32 [S, D], v int64 [S, K]) of the selected rows (None: all, in order)."""
    v = factor_values(lat_sizes)
    assert table.shape[0] == v.shape[0], (table.shape, lat_sizes)
    if rows is None:
        return table, v
    return table[rows], v[rows]


FAMILIES = ("gauss", "disent", "const", "ties", "offset")


def make_table(lat_sizes, D, family, seed=0):
    """fp32 [N, D].  gauss: columns of different scale and offset; disent: column d = factor d % K + 1e-3 noise (64 consecutive
    rows of a slow factor land in one bin); const: every column one value; ties: integers 0 .. 20 (exactly the edges of 20 bins);
    offset: gauss with + 30 on column D // 2 (tests/test_gpu_factor_scores.py)."""
    assert family in FAMILIES, family
    v = factor_values(lat_sizes)
    N, K = v.shape
    rng = np.random.default_rng(seed + 1000 * D + N)
    if family in ("gauss", "offset"):
        t = rng.standard_normal((N, D)) * rng.uniform(0.01, 2.0, size=D) + rng.uniform(-1, 1, size=D)
        if family == "offset":
            t[:, D // 2] += 30.0
    elif family == "disent":
        t = v[:, np.arange(D) % K] + 1e-3 * rng.standard_normal((N, D))
    elif family == "const":
        t = np.broadcast_to(rng.uniform(-3, 3, size=D), (N, D))
    else:
        t = rng.integers(0, 21, size=(N, D))
    return np.ascontiguousarray(t.astype(np.float32))


def ideal_table(lat_sizes, D):
    """z_k = v_k exactly for k < K, the other D - K columns constant."""
    v = factor_values(lat_sizes)
    t = np.full((v.shape[0], D), 0.25, dtype=np.float32)
    t[:, :v.shape[1]] = v
    return t


def rotated_table(lat_sizes, D):
    """ideal_table with columns 0 and 1 (standardised) rotated by 45 degrees: two latents share two factors."""
    t = ideal_table(lat_sizes, D).astype(np.float64)
    a, b = (t[:, i] / t[:, i].std() for i in (0, 1))
    t[:, 0], t[:, 1] = (a + b) / np.sqrt(2.0), (a - b) / np.sqrt(2.0)
    return t.astype(np.float32)


# ---- histograms -----------------------------------------------------------------------------------------------------------------
def lower_edges(x, n_bins):
    """the n_bins lower bin edges of numpy.histogram(x, n_bins) for an fp32 column (fp32, as numpy returns them)."""
    edges = np.histogram(x, bins=n_bins)[1]
    assert edges.dtype == np.float32 and edges.shape == (n_bins + 1,), (edges.dtype, edges.shape)
    return edges[:-1]


def bins_of(x, edges):
    return np.clip(np.digitize(x, edges) - 1, 0, len(edges) - 1)


def joint_counts(table, lat_sizes, n_bins, rows=None):
    """-> (counts int64 [D, n_bins * sum(lat_sizes)] in the layout of dvae_info_joint_hist, edges fp32 [D, n_bins])."""
    x, v = select(table, lat_sizes, rows)
    D, sizes = x.shape[1], [int(s) for s in lat_sizes]
    counts, edges = np.zeros((D, n_bins * sum(sizes)), dtype=np.int64), np.zeros((D, n_bins), dtype=np.float32)
    for d in range(D):
        edges[d] = lower_edges(x[:, d], n_bins)
        b = bins_of(x[:, d], edges[d])
        start = 0
        for k, size in enumerate(sizes):
            block = np.bincount(b * size + v[:, k], minlength=n_bins * size)
            counts[d, start:start + n_bins * size] = block
            start += n_bins * size
    return counts, edges


def blocks_of(counts_d, lat_sizes, n_bins):
    """one latent's counters -> the K blocks [n_bins, lat_sizes[k]]."""
    out, start = [], 0
    for size in lat_sizes:
        out.append(counts_d[start:start + n_bins * size].reshape(n_bins, size))
        start += n_bins * size
    return out


# ---- moments --------------------------------------------------------------------------------------------------------------------
def moments(table, lat_sizes, rows=None):
    """fp64: min, max (the fp32 elements), mean [D], var [D], cov [D, K], factor_mean [K], factor_var [K], and absmax of the
    columns / factors; numpy.cov with ddof = 1, zeros when one row is selected."""
    x, v = select(table, lat_sizes, rows)
    S, D, K = x.shape[0], x.shape[1], v.shape[1]
    x64, v64 = x.astype(np.float64), v.astype(np.float64)
    if S > 1:
        c = np.atleast_2d(np.cov(np.concatenate([x64.T, v64.T]), ddof=1))
    else:
        c = np.zeros((D + K, D + K))
    return {"min": x.min(axis=0), "max": x.max(axis=0), "mean": x64.mean(axis=0), "var": np.diag(c)[:D].copy(), "cov": c[:D, D:].copy(),
            "factor_mean": v64.mean(axis=0), "factor_var": np.diag(c)[D:].copy(), "absmax": np.abs(x64).max(axis=0),
            "factor_absmax": np.abs(v64).max(axis=0)}


def moments32(table, lat_sizes, rows=None):
    """the same centred sums in fp32 (shift by the first selected row, mean, deviations), numpy's pairwise sums."""
    x, v = select(table, lat_sizes, rows)
    S = x.shape[0]
    f = np.float32
    x, v = np.ascontiguousarray(x.astype(f).T), np.ascontiguousarray(v.astype(f).T)      # [D, S], [K, S]: sums run along the
    dx, dv = x - x[:, :1], v - v[:, :1]                                                   # contiguous axis, where numpy's are pairwise
    mx, mv = dx.sum(axis=1, dtype=f) / f(S), dv.sum(axis=1, dtype=f) / f(S)
    ex, ev = dx - mx[:, None], dv - mv[:, None]
    n1 = f(max(S - 1, 1))
    cov = np.stack([(ex * ev[k]).sum(axis=1, dtype=f) for k in range(v.shape[0])], axis=1) / n1
    return {"mean": x[:, 0] + mx, "var": (ex * ex).sum(axis=1, dtype=f) / n1, "cov": cov,
            "factor_mean": v[:, 0] + mv, "factor_var": (ev * ev).sum(axis=1, dtype=f) / n1}


def pair_tolerance(s_i, s_j, a_i, a_j):
    return 1e-5 * s_i * s_j + 4 * 2.0 ** -24 * (a_i * s_j + a_j * s_i) / 2


def mean_tolerance(s, a):
    return 1e-5 * s + 4 * 2.0 ** -24 * a


def moment_tolerances(ref):
    s, a = np.sqrt(ref["var"]), ref["absmax"]
    sf, af = np.sqrt(ref["factor_var"]), ref["factor_absmax"]
    return {"mean": mean_tolerance(s, a), "var": pair_tolerance(s, s, a, a),
            "cov": pair_tolerance(s[:, None], sf[None, :], a[:, None], af[None, :]),
            "factor_mean": mean_tolerance(sf, af), "factor_var": pair_tolerance(sf, sf, af, af)}


def worst_ratio(got, ref, tol):
    """max |got - ref| / tol; a zero tolerance (a constant column, one row) asks for the exact value."""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    if not np.isfinite(err).all():
        return float("inf")
    ratio = np.where(err == 0, 0.0, err / np.where(tol > 0, tol, 1e-300))
    return float(ratio.max()) if ratio.size else 0.0


def moment_ratios(got, ref):
    tol = moment_tolerances(ref)
    return {k: worst_ratio(got[k], ref[k], tol[k]) for k in tol}


# ---- scores ---------------------------------------------------------------------------------------------------------------------
def mutual_information(block):
    """sklearn.metrics.mutual_info_score of a contingency table: sum over the nonzero cells of P log(P / (P_row P_col)), nats."""
    block = np.asarray(block, dtype=np.float64)
    S, row, col = block.sum(), block.sum(axis=1, keepdims=True), block.sum(axis=0, keepdims=True)
    # P / (P_row P_col) = c S / (row col), formed from the integer counts: both products are exact in fp64, so a cell of an
    # independent table (a constant latent: row = S) contributes log(1) = 0 exactly and "no information" stays the number 0
    ratio = (block * S) / (row * col).clip(min=1)
    nz = block > 0
    return float((block[nz] / S * np.log(ratio[nz])).sum())


def entropy(p):
    p = np.asarray(p, dtype=np.float64)
    p = p[p > 0] / p.sum()
    return float(-(p * np.log(p)).sum())


def _gap(m):
    ranked = np.sort(m, axis=0)[::-1]
    return ranked[0] - (ranked[1] if m.shape[0] > 1 else 0.0)


def scores(table, lat_sizes, n_bins=20, rows=None):
    sizes = [int(s) for s in lat_sizes]
    x, v = select(table, sizes, rows)
    D, K = x.shape[1], len(sizes)
    counts, _ = joint_counts(table, sizes, n_bins, rows)
    mi = np.array([[mutual_information(b) for b in blocks_of(counts[d], sizes, n_bins)] for d in range(D)])
    H = np.array([entropy(np.bincount(v[:, k], minlength=sizes[k])) for k in range(K)])
    if not (H > 0).all():
        raise ValueError("a factor without entropy")
    m = mi ** 2
    t = m.max(axis=1)
    mod = np.zeros(D)
    for d in range(D):
        if t[d] > 0:
            mod[d] = 1.0 if K == 1 else 1.0 - (m[d].sum() - t[d]) / (t[d] * (K - 1))
    mom = moments(table, sizes, rows)
    sap = np.zeros((D, K))
    live = mom["var"] > 1e-12
    sap[live] = mom["cov"][live] ** 2 / (mom["var"][live, None] * mom["factor_var"][None, :])
    return {"mig_discrete": float(np.mean(_gap(mi) / H)), "modularity": float(mod.mean()), "sap_continuous": float(np.mean(_gap(sap))),
            "sap_matrix": sap, "mutual_information": mi, "factor_entropy": H, "n_samples": x.shape[0], "n_bins": n_bins}


# ---- the shapes of tests/test_gpu_information_scores.py (here: tests/test_information_scores_host.py pins their e32 on the CPU) ----
_L = [(60,), (3, 4, 5), (2, 3, 6, 40), (3, 6, 40, 32), (1000, 3), (2, 2, 2, 2, 2, 2, 2, 2)]
# (lat_sizes, D, n_bins, family): every D of {1, 3, 10, 17, 64} and every lat_sizes at least twice, every n_bins of {2, 20, 64}, every
# family four times.  (1000, 3) at 20 / 64 bins has more counters per latent than the LDS histogram holds, at 2 bins it fits.
CASES = [(_L[0], 1, 20, "gauss"), (_L[0], 10, 2, "disent"), (_L[0], 64, 64, "ties"),
         (_L[1], 3, 20, "ties"), (_L[1], 17, 64, "gauss"), (_L[1], 10, 20, "const"),
         (_L[2], 10, 20, "disent"), (_L[2], 1, 64, "offset"), (_L[2], 64, 2, "gauss"),
         (_L[3], 10, 20, "disent"), (_L[3], 3, 64, "gauss"), (_L[3], 17, 20, "offset"),
         (_L[4], 10, 20, "gauss"), (_L[4], 3, 2, "disent"), (_L[4], 1, 64, "const"), (_L[4], 17, 20, "ties"),
         (_L[5], 64, 20, "disent"), (_L[5], 3, 2, "const"), (_L[5], 10, 64, "offset"), (_L[5], 1, 20, "ties")]
SELECTIONS = (None, 1, 63, 65, 10000)                       # all rows in order; S random rows with repeats


def switch_cases(lib):
    """(lat_sizes, D, n_bins, family, S): the last shape below and the first above every dispatch macro of include/dvae_info_hip.h
    (lib = disvae_amd._infolib, which mirrors them).  Large S on a 60-row table: the rows repeat, the table stays small."""
    out = []
    for lanes in (lib.ROW_LANES_NARROW, lib.ROW_LANES_MID, lib.ROW_LANES_WAVE):              # lanes per row of the moments pass
        out += [(_L[1], lanes, 20, "gauss", None), (_L[1], lanes + 1, 20, "gauss", None)]
    for rows in (lib.MOMENTS_BLOCK_ROWS, lib.HIST_BLOCK_ROWS):                               # one workgroup / two
        out += [(_L[1], 3, 20, "offset", rows), (_L[1], 3, 20, "offset", rows + 1)]
    for rows in (lib.MOMENTS_BLOCK_ROWS * lib.MAX_BLOCKS, lib.HIST_BLOCK_ROWS * lib.MAX_BLOCKS):   # the grid stops growing
        out += [(_L[0], 1, 20, "gauss", rows), (_L[0], 1, 20, "gauss", rows + 1)]
    side = int(lib.HIST_LDS_INTS // lib.MAX_BINS) // 2                                       # n_bins * sum(lat_sizes) = the LDS limit
    out += [((side, side), 3, lib.MAX_BINS, "gauss", None), ((side, side + 1), 3, lib.MAX_BINS, "gauss", None)]
    return out


@functools.lru_cache(maxsize=None)
def case(lat_sizes, D, n_bins, family, S):
    """Table, rows (None: all; else S random rows with repeats) and the fp64 statistics: computed once, shared, never modified."""
    table = make_table(lat_sizes, D, family)
    rows = None
    if S is not None:
        rows = np.random.default_rng(S + D).integers(0, table.shape[0], size=S)
    counts, edges = joint_counts(table, lat_sizes, n_bins, rows)
    return {"table": table, "rows": rows, "counts": counts, "edges": edges, "moments": moments(table, lat_sizes, rows),
            "moments32": moments32(table, lat_sizes, rows)}
