"""fp64 numpy restatement of the interventional robustness score (Suter et al. 2019; disentanglement_lib's irs.py) and of the two
statistics under it (a helper module, like info_ref.py): what Evaluator.compute_irs and the kernels of csrc/factor_irs.hip are
judged by.  Written from the definition, independent of disvae_amd/evaluate.py: the factor values are materialised with
numpy.indices, groups are boolean masks, the discretiser is numpy.histogram + numpy.digitize literally, the quantile is
numpy.percentile, the order statistics are numpy.sort.

The end-to-end bound of tests/test_gpu_irs.py lives here too, so that tests/test_irs_host.py can pin its precondition without a
GPU: every entry of IRS_matrix within 4 * 2^-24 * max|table| / max_deviations[d] of the fp64 restatement (a centre that is one
fp32 ulp off moves a deviation by at most that ulp, and the matrix divides by max_deviations); the restatement with fp32-rounded
centres and fp32 deviations must itself stay within a QUARTER of that.
"""
import functools

import numpy as np

import info_ref as I

Q = 0.99


# ---- step 1: the groups ---------------------------------------------------------------------------------------------------------
def bin_labels(size, factor_bins):
    """the label of every value 0 .. size - 1 of one factor: the value itself, or its numpy.digitize bin on the edges of the
    factor's full range (labels are NOT relabelled here: numpy.unique on what is present does that)."""
    values = np.arange(size)
    if factor_bins is None:
        return values
    return np.digitize(values, np.histogram(values, factor_bins)[1][:-1])


def group_layout(lat_sizes, factor_bins):
    """-> (group_of_value int32 [sum(lat_sizes)], n_groups [K]) with the distinct labels of a factor relabelled 0 .. G - 1."""
    parts, n_groups = [], []
    for size in lat_sizes:
        dense = np.unique(bin_labels(int(size), factor_bins), return_inverse=True)[1].reshape(-1)
        parts.append(dense.astype(np.int32))
        n_groups.append(int(dense.max()) + 1)
    return np.concatenate(parts), n_groups


def group_masks(lat_sizes, factor_bins, rows=None):
    """bool [total_groups, S] in the group index space of include/dvae_irs_hip.h: slot 0 = every selected row, then factor by factor."""
    v = I.factor_values(lat_sizes)
    if rows is not None:
        v = v[rows]
    gmap, n_groups = group_layout(lat_sizes, factor_bins)
    masks, off = [np.ones(v.shape[0], dtype=bool)], 0
    for k, size in enumerate(lat_sizes):
        g = gmap[off + v[:, k]]
        masks += [g == i for i in range(n_groups[k])]
        off += int(size)
    return np.stack(masks), n_groups


# ---- steps 2 to 6, literally ----------------------------------------------------------------------------------------------------
def irs(table, lat_sizes, diff_quantile=Q, factor_bins=20, rows=None, fp32_path=False):
    """The score.  fp32_path: the centres rounded to fp32 and the deviations formed in fp32 (what the kernels do); else all fp64."""
    x, v = I.select(table, lat_sizes, rows)
    x64 = x.astype(np.float64)
    D, K = x.shape[1], len(lat_sizes)

    def deviations(mask):
        c = x64[mask].mean(axis=0)
        if fp32_path:
            return np.abs(x[mask].astype(np.float32) - c.astype(np.float32)).astype(np.float64)
        return np.abs(x64[mask] - c)
    max_deviations = deviations(np.ones(x.shape[0], dtype=bool)).max(axis=0)
    active = max_deviations > 0
    matrix = np.zeros((D, K))
    for k, size in enumerate(lat_sizes):
        labels = bin_labels(int(size), factor_bins)[v[:, k]]
        present = np.unique(labels)
        max_diffs = np.stack([np.percentile(deviations(labels == u), 100 * diff_quantile, axis=0) for u in present])
        matrix[active, k] = 1.0 - max_diffs.mean(axis=0)[active] / max_deviations[active]
    matrix = matrix[active]
    if not active.any():
        return {"IRS": 0.0, "disentanglement_scores": np.zeros(0), "parents": np.zeros(0, dtype=np.int64), "IRS_matrix": matrix,
                "max_deviations": max_deviations, "active": active}
    scores = matrix.max(axis=1)
    return {"IRS": float(np.average(scores, weights=max_deviations[active])), "disentanglement_scores": scores,
            "parents": matrix.argmax(axis=1), "IRS_matrix": matrix, "max_deviations": max_deviations, "active": active}


def matrix_bound(table, ref):
    """[A] per active latent: 4 * 2^-24 * max|table| / max_deviations[d]."""
    return 4 * 2.0 ** -24 * float(np.abs(table.astype(np.float64)).max()) / ref["max_deviations"][ref["active"]]


def worst_ratio(got, ref, bound):
    """max over IRS_matrix, disentanglement_scores and IRS of |got - ref| / bound (the scalar against the largest bound)."""
    assert np.array_equal(got["active"], ref["active"]), (got["active"], ref["active"])
    if not ref["active"].any():
        return 0.0 if got["IRS"] == 0.0 else float("inf")
    r = [np.abs(got["IRS_matrix"] - ref["IRS_matrix"]).max(axis=1) / bound,
         np.abs(got["disentanglement_scores"] - ref["disentanglement_scores"]) / bound,
         [abs(got["IRS"] - ref["IRS"]) / bound.max()]]
    return float(max(np.max(a) for a in r))


# ---- the two statistics ---------------------------------------------------------------------------------------------------------
def group_means(table, lat_sizes, factor_bins, rows=None):
    """-> counts int64 [G], means fp64 [G, D] (0 for an empty group), span fp64 [D] = max |x - x_0| over the selected rows."""
    x, _ = I.select(table, lat_sizes, rows)
    x64 = x.astype(np.float64)
    masks, n_groups = group_masks(lat_sizes, factor_bins, rows)
    counts = masks.sum(axis=1)
    means = np.stack([x64[m].mean(axis=0) if m.any() else np.zeros(x.shape[1]) for m in masks])
    return counts, means, np.abs(x64 - x64[0]).max(axis=0), n_groups


def ulp32(v):
    v = np.abs(np.asarray(v, dtype=np.float64)).astype(np.float32)
    return (np.nextafter(v, np.float32(np.inf)) - v).astype(np.float64)


def mean_tolerance(ref64, counts, span):
    """|got - ref64| <= 0.5 ulp32(ref64) (1 + 1e-6) + n_g 2^-52 max|x - x_0|: the final rounding plus n_g fp64 additions."""
    return 0.5 * ulp32(ref64) * (1 + 1e-6) + counts[:, None] * 2.0 ** -52 * span[None, :]


def sorted_deviations(table, lat_sizes, factor_bins, centres, rows=None):
    """per group the fp32 |x - centre| of its rows, sorted along the rows by numpy.sort: a list of fp32 [n_g, D]."""
    x, _ = I.select(table, lat_sizes, rows)
    masks, _ = group_masks(lat_sizes, factor_bins, rows)
    out = [np.sort(np.abs(x[m].astype(np.float32) - centres[g].astype(np.float32)[None, :]), axis=0) for g, m in enumerate(masks)]
    assert all(d.dtype == np.float32 for d in out)
    return out


def order_stats(sorted_devs, ranks):
    """The rank-th and (rank + 1)-th smallest and the largest deviation of every group: fp32 [G, D] each; zeros where the rank is
    outside [0, n_g)."""
    G, D = len(sorted_devs), sorted_devs[0].shape[1]
    lo, hi, mx = (np.zeros((G, D), dtype=np.float32) for _ in range(3))
    for g, dev in enumerate(sorted_devs):
        n, k = dev.shape[0], int(ranks[g])
        if 0 <= k < n:
            lo[g], hi[g], mx[g] = dev[k], dev[min(k + 1, n - 1)], dev[n - 1]
    return lo, hi, mx


def quantile_rank(n, q):
    return int(np.floor((n - 1) * (100.0 * q / 100.0))) if n > 0 else -1


def rank_sets(counts, q=Q):
    """the four ranks per group the GPU tests ask for: 0, n - 1, the q-quantile's and a middle one (-1 for an empty group)."""
    c = np.asarray(counts)
    return {"first": np.where(c > 0, 0, -1), "last": c - 1, "quantile": np.array([quantile_rank(int(n), q) for n in c]),
            "middle": np.where(c > 0, c // 2, -1)}


# ---- the shapes of tests/test_gpu_irs.py ------------------------------------------------------------------------------------------
_L = [(60,), (3, 4, 5), (2, 3, 6, 20)]
# (lat_sizes, D, family, factor_bins): every lat_sizes, every D of {1, 3, 10, 17, 64} and every family at least once
CASES = [(_L[0], 1, "gauss", 20), (_L[0], 10, "disent", None), (_L[0], 64, "ties", 7),
         (_L[1], 3, "ties", 20), (_L[1], 17, "gauss", 20), (_L[1], 10, "const", 20), (_L[1], 1, "offset", None),
         (_L[2], 10, "disent", 20), (_L[2], 64, "gauss", 4), (_L[2], 17, "offset", 20), (_L[2], 3, "const", None)]
SELECTIONS = (None, 1, 63, 65, 10000)                       # all rows in order; S random rows with repeats


def switch_cases(lib):
    """(lat_sizes, D, family, factor_bins, S): the last shape below and the first above every dispatch macro of
    include/dvae_irs_hip.h (lib = disvae_amd._irslib, which mirrors them).  Large S on a 60-row table: the rows repeat."""
    out = [(_L[1], lib.MEANS_COLS, "gauss", 20, None), (_L[1], lib.MEANS_COLS + 1, "gauss", 20, None)]
    for rows in (lib.MEANS_BLOCK_ROWS, lib.SELECT_BLOCK_ROWS):                               # one workgroup / two
        out += [(_L[1], 3, "offset", 20, rows), (_L[1], 3, "offset", 20, rows + 1)]
    for rows in (lib.MEANS_BLOCK_ROWS * lib.MAX_BLOCKS, lib.SELECT_BLOCK_ROWS * lib.MAX_BLOCKS):   # the grid stops growing
        out += [(_L[0], 1, "gauss", 20, rows), (_L[0], 1, "gauss", 20, rows + 1)]
    g = lib.SELECT_LDS_GROUPS                                                                # one slice of groups / two
    out += [((g, 3), 3, "gauss", None, None), ((g + 1, 3), 3, "gauss", None, None)]
    out += [((183, 2), 3, "disent", None, None), ((lib.MAX_GROUPS, 2), 2, "gauss", None, None)]   # five slices; the limit itself
    return out


def rows_of(n_table, D, S):
    return None if S is None else np.random.default_rng(S + D).integers(0, n_table, size=S)


@functools.lru_cache(maxsize=None)
def case(lat_sizes, D, family, factor_bins, S):
    """Table, rows, the group layout and the fp64 statistics: computed once, shared, never modified."""
    table = I.make_table(lat_sizes, D, family)
    rows = rows_of(table.shape[0], D, S)
    counts, means, span, n_groups = group_means(table, lat_sizes, factor_bins, rows)
    gmap, _ = group_layout(lat_sizes, factor_bins)
    return {"table": table, "rows": rows, "counts": counts, "means": means, "span": span, "n_groups": n_groups, "gmap": gmap,
            "centres": means.astype(np.float32)}


# ---- the end-to-end cases (tests/test_gpu_irs.py; their precondition: tests/test_irs_host.py) ----------------------------------
def end_to_end_table(kind, lat_sizes, D):
    if kind == "ideal":
        return I.ideal_table(lat_sizes, D)
    if kind == "rotated":
        return I.rotated_table(lat_sizes, D)
    return I.make_table(lat_sizes, D, kind)


# (kind, lat_sizes, D, factor_bins, diff_quantile, S)
END_TO_END = [("ideal", (3, 4, 5), 5, 20, Q, None), ("ideal", (2, 3, 6, 20), 7, 20, Q, None),
              ("rotated", (3, 4, 5), 3, 20, Q, None), ("rotated", (2, 3, 6, 20), 7, 20, Q, None),
              ("gauss", (3, 4, 5), 3, 20, Q, None), ("gauss", (2, 3, 6, 20), 7, 20, Q, None),
              ("gauss", (2, 3, 6, 20), 10, 4, 0.5, 500), ("disent", (2, 3, 6, 20), 10, None, Q, None),
              ("ties", (3, 4, 5), 17, 20, 1.0, None), ("const", (3, 4, 5), 10, 20, Q, None), ("gauss", (60,), 1, 20, 0.0, 10000)]
