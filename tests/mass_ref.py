"""fp64 restatement of the posterior mass table and of the RMIG / JEMMIG / MIG-sup / DCIMIG scores built on it
(include/dvae_mass_hip.h, evaluate.interpretability_scores_from_mass), in numpy plus math.erfc only: a plain helper module, like
sep_ref.py.  Everything is written out literally -- one row, one latent, one bin at a time where that is the definition.

Definitions (Do & Tran 2020 for RMIG / JEMMIG; Li et al. 2020 for MIG-sup; Sepliarskaia et al. 2019 for DCIMIG):
    edges   e = numpy.linspace(lo, hi, nb + 1)[1:-1]; bin 0 = (-inf, e_1), bin nb - 1 = [e_{nb-1}, +inf)
    sigma = exp(logvar / 2),  t_j = (e_j - mean) / (sigma sqrt 2),  up_j = erfc(t_j) / 2,  dn_j = erfc(-t_j) / 2
    Q_0 = dn_1,  Q_{nb-1} = up_{nb-1},  Q_b = up_b - up_{b+1} if t_b >= 0 else dn_{b+1} - dn_b          (nb = 1: Q_0 = 1)
    mass[d][k][b, v] = sum over the selected rows s with v_k(rows[s]) = v of Q_b(rows[s], d),  v_k(r) = (r // stride_k) % lat_sizes[k]
"""
import math

import numpy as np

# The worst error of math.erfc, in ulps of the true value, over the arguments the test tables produce: measured against mpmath at 40
# digits by tests/test_mass_host.py (2.996 there), which holds this pin.  The per-cell bound of the GPU test is built from it.
U_REF = 3.0
SQRT2 = math.sqrt(2.0)
_erfc = np.vectorize(math.erfc, otypes=[np.float64])
_erf = np.vectorize(math.erf, otypes=[np.float64])


def edges(n_bins, z_range=(-4.0, 4.0)):
    return np.linspace(float(z_range[0]), float(z_range[1]), int(n_bins) + 1)[1:-1].astype(np.float64)


def scaled_edges(mu, lv, e):
    """t_j for one fp32 (mean, logvar) pair and the edges e: [nb - 1] fp64."""
    sigma = math.exp(float(lv) / 2.0)
    return (e - float(mu)) / (sigma * SQRT2)


def row_masses(mu, lv, e):
    """Q [nb] of one posterior N(mu, exp(lv)): the definition, one bin at a time."""
    nb = len(e) + 1
    if nb == 1:
        return np.ones(1)
    t = [None] + list(scaled_edges(mu, lv, e))                     # t[1] .. t[nb - 1]
    up = lambda j: 0.5 * math.erfc(t[j])                           # noqa: E731
    dn = lambda j: 0.5 * math.erfc(-t[j])                          # noqa: E731
    Q = np.zeros(nb)
    Q[0] = dn(1)
    Q[nb - 1] = up(nb - 1)
    for b in range(1, nb - 1):
        Q[b] = up(b) - up(b + 1) if t[b] >= 0 else dn(b + 1) - dn(b)
    return Q


def masses(mean, logvar, e):
    """Q [N, D, nb] of every (row, latent): row_masses, vectorised over the table (the same operations in the same order)."""
    mean, logvar = np.asarray(mean), np.asarray(logvar)
    nb = len(e) + 1
    if nb == 1:
        return np.ones(mean.shape + (1,))
    sigma = np.exp(logvar.astype(np.float64) / 2.0)
    t = (e[None, None, :] - mean.astype(np.float64)[:, :, None]) / (sigma * SQRT2)[:, :, None]      # [N, D, nb - 1]: t_1 ..
    up, dn = 0.5 * _erfc(t), 0.5 * _erfc(-t)
    Q = np.zeros(mean.shape + (nb,))
    Q[:, :, 0] = dn[:, :, 0]
    Q[:, :, nb - 1] = up[:, :, nb - 2]
    if nb > 2:
        Q[:, :, 1:nb - 1] = np.where(t[:, :, :-1] >= 0, up[:, :, :-1] - up[:, :, 1:], dn[:, :, 1:] - dn[:, :, :-1])
    return Q


def masses_erf_form(mean, logvar, e):
    """The form the header forbids: Phi(b) - Phi(a) with Phi = (1 + erf) / 2 (the end bins Phi(e_1) and 1 - Phi(e_{nb-1}))."""
    sigma = np.exp(np.asarray(logvar, dtype=np.float64) / 2.0)
    t = (e[None, None, :] - np.asarray(mean, dtype=np.float64)[:, :, None]) / (sigma * SQRT2)[:, :, None]
    phi = 0.5 * (1.0 + _erf(t))
    full = np.concatenate([np.zeros(phi.shape[:2] + (1,)), phi, np.ones(phi.shape[:2] + (1,))], axis=2)
    return full[:, :, 1:] - full[:, :, :-1]


def factor_values(rows, lat_sizes):
    """v [S, K] of the row numbers `rows` of a data set that enumerates lat_sizes in row-major order."""
    rows = np.asarray(rows, dtype=np.int64)
    v = np.zeros((len(rows), len(lat_sizes)), dtype=np.int64)
    stride = 1
    for k in range(len(lat_sizes) - 1, -1, -1):
        v[:, k] = (rows // stride) % lat_sizes[k]
        stride *= lat_sizes[k]
    return v


def mass_table(mean, logvar, lat_sizes, n_bins, z_range=(-4.0, 4.0), rows=None):
    """-> (mass [D, n_bins * sum(lat_sizes)] in the layout of dvae_mass_joint, n_v [sum(lat_sizes)]: how many selected rows
    carry each value of each factor).  Every cell is the EXACT sum of its rows' fp64 masses rounded once (math.fsum), so the
    reference adds no error of an order of summation to the per-row bound: a running fp64 sum of 8192 rows drawn from 24 distinct ones
    is off by 12 of those bounds, its roundings all falling the same way (measured; the device's chunked order by 0.4)."""
    N, D = mean.shape
    rows = np.arange(N) if rows is None else np.asarray(rows, dtype=np.int64)
    Q = masses(mean, logvar, edges(n_bins, z_range))             # [N, D, nb]
    v = factor_values(rows, lat_sizes)
    blocks, counts = [], []
    for k, size in enumerate(lat_sizes):
        block = np.zeros((D, n_bins, size))
        for value in range(size):
            carried = Q[rows[v[:, k] == value]]                  # [n_v, D, nb], in the order of `rows`
            for d in range(D):
                for b in range(n_bins):
                    block[d, b, value] = math.fsum(carried[:, d, b])
        blocks.append(block.reshape(D, n_bins * size))
        counts.append(np.bincount(v[:, k], minlength=size))
    return np.concatenate(blocks, axis=1), np.concatenate(counts)


def cell_counts(n_v, lat_sizes, n_bins):
    """n_v spread over one latent's [n_bins * sum(lat_sizes)] cells: the number of rows summed into each."""
    out, start = [], 0
    for size in lat_sizes:
        out.append(np.tile(n_v[start:start + size], n_bins))
        start += size
    return np.concatenate(out)


def scores(mass, lat_sizes, n_bins):
    """The scores of interpretability_scores_from_mass, with loops where the definition has an index."""
    D, K = mass.shape[0], len(lat_sizes)
    I, Hj, Hy, Hz = np.zeros((D, K)), np.zeros((D, K)), np.zeros(K), np.zeros(D)
    start = 0
    for k, size in enumerate(lat_sizes):
        for d in range(D):
            P = mass[d, start:start + n_bins * size].reshape(n_bins, size)
            P = P / P.sum()
            Pz, Pv = P.sum(axis=1), P.sum(axis=0)
            for b in range(n_bins):
                for v in range(size):
                    if P[b, v] > 0:
                        I[d, k] += P[b, v] * math.log(P[b, v] / Pz[b] / Pv[v])     # (not / (Pz Pv): that product underflows first)
                        Hj[d, k] -= P[b, v] * math.log(P[b, v])
            if d == 0:
                Hy[k] = -sum(p * math.log(p) for p in Pv if p > 0)
            if k == 0:
                Hz[d] = -sum(p * math.log(p) for p in Pz if p > 0)
        start += n_bins * size
    if min(Hy) <= 0:
        raise ValueError("a factor without entropy")
    rmig, jemmig, jemmig_norm, best = np.zeros(K), np.zeros(K), np.zeros(K), np.zeros(K, dtype=np.int64)
    for k in range(K):
        i = max(range(D), key=lambda d: (I[d, k], -d))               # the lowest d on ties
        second = max([I[d, k] for d in range(D) if d != i], default=0.0)
        best[k], rmig[k] = i, I[i, k] - second
        jemmig[k] = Hj[i, k] - I[i, k] + second
        jemmig_norm[k] = 1.0 - jemmig[k] / (Hy[k] + math.log(n_bins))
    mig_sup, gap, prefers = np.zeros(D), np.zeros(D), np.zeros(D, dtype=np.int64)
    for d in range(D):
        norm = sorted((I[d, k] / Hy[k] for k in range(K)), reverse=True)
        raw = sorted((I[d, k] for k in range(K)), reverse=True)
        mig_sup[d] = norm[0] - (norm[1] if K > 1 else 0.0)
        gap[d] = raw[0] - (raw[1] if K > 1 else 0.0)
        prefers[d] = max(range(K), key=lambda k: (I[d, k], -k))
    dcimig = sum(max([gap[d] for d in range(D) if prefers[d] == k], default=0.0) for k in range(K)) / Hy.sum()
    return {"rmig": float(rmig.mean()), "rmig_norm": float((rmig / Hy).mean()), "jemmig": float(jemmig.mean()),
            "jemmig_norm": float(jemmig_norm.mean()), "mig_sup": float(mig_sup.mean()), "dcimig": float(dcimig),
            "rmig_per_factor": rmig, "jemmig_per_factor": jemmig, "jemmig_norm_per_factor": jemmig_norm,
            "mig_sup_per_latent": mig_sup, "best_latent": best, "factor_entropy": Hy, "latent_entropy": Hz,
            "mutual_information": I, "joint_entropy": Hj}


SCALAR_SCORES = ("rmig", "rmig_norm", "jemmig", "jemmig_norm", "mig_sup", "dcimig")


def score_bound(mass, cell_bound, lat_sizes, n_bins):
    """How far the scores can move when every cell of `mass` moves by at most `cell_bound` (same shape), to first order: an
    entropy is a sum of -P log P, whose derivative is -(log P + 1), so a block's entropies move by at most the sum over its cells
    with P > 0 of |log P + 1| * cell_bound / S.  Returned: that sum over ALL cells of the table, every block a score draws on
    included."""
    D, total, start = mass.shape[0], 0.0, 0
    for size in lat_sizes:
        for d in range(D):
            block, cb = mass[d, start:start + n_bins * size], cell_bound[d, start:start + n_bins * size]
            S = block.sum()
            nz = block / S > 0                                           # (a subnormal mass can round to P = 0: no term, as in scores)
            total += float((np.abs(np.log(block[nz] / S) + 1.0) * cb[nz]).sum() / S)
        start += n_bins * size
    return total


# ---- tables ------------------------------------------------------------------------------------------------------------------------
FAMILIES = ("broad", "sharp", "wide", "far", "edge", "tiny")


def table(family, N, D, n_bins, seed, z_range=(-4.0, 4.0)):
    """fp32 (mean, logvar) [N, D].  broad: logvar about 0;  sharp: logvar -12, a row's mass in one or two bins;  wide: logvar +4, most
    mass in the two tail bins;  far: means at +-30, everything in a tail bin;  edge: means exactly on an edge (those fp32 can hold),
    sharp and broad rows mixed;  tiny: logvar -20."""
    rng = np.random.RandomState(seed)
    mean = rng.uniform(-3.5, 3.5, (N, D))
    if family == "broad":
        logvar = rng.uniform(-1.0, 1.0, (N, D))
    elif family == "sharp":
        logvar = -12.0 + rng.uniform(-0.5, 0.5, (N, D))
    elif family == "wide":
        logvar = 4.0 + rng.uniform(-0.5, 0.5, (N, D))
    elif family == "far":
        mean = np.where(rng.rand(N, D) < 0.5, -30.0, 30.0) + rng.uniform(-1.0, 1.0, (N, D))
        logvar = rng.uniform(-14.0, 0.0, (N, D))
    elif family == "edge":
        e = edges(max(n_bins, 2), z_range)
        mean = e[rng.randint(0, len(e), (N, D))].astype(np.float32).astype(np.float64)
        logvar = np.where(rng.rand(N, D) < 0.5, -12.0, 0.0) + rng.uniform(-0.5, 0.5, (N, D))
    elif family == "tiny":
        logvar = np.full((N, D), -20.0)
    else:
        raise ValueError(family)
    return mean.astype(np.float32), logvar.astype(np.float32)


def far_sharp_table(seed=0):
    """720 + 720 rows of one latent: means up to 30 outside z_range = (-4, 4) with logvar down to -14, then means inside the range
    with the same logvars -- the table on which Phi(b) - Phi(a) loses every small cell."""
    rng = np.random.RandomState(seed)
    far = np.where(rng.rand(720) < 0.5, -1.0, 1.0) * rng.uniform(4.0, 34.0, 720)
    mean = np.concatenate([far, rng.uniform(-4.0, 4.0, 720)])[:, None]
    logvar = rng.uniform(-14.0, 0.0, (1440, 1))
    return mean.astype(np.float32), logvar.astype(np.float32)


GRID = (6, 5, 4, 3, 2)


def _standardised_factors(lat_sizes):
    v = factor_values(np.arange(int(np.prod(lat_sizes))), lat_sizes).astype(np.float64)
    return (v - v.mean(axis=0)) / v.std(axis=0)


def ideal_table(seed=0, lat_sizes=GRID):
    """D = K + 2: latent k is 1.5 x the standardised factor k with logvar -8 + 0.1 noise; two collapsed latents, mean 0.01 noise,
    logvar 0."""
    rng = np.random.RandomState(seed)
    f = _standardised_factors(lat_sizes)
    N, K = f.shape
    mean = np.concatenate([1.5 * f, 0.01 * rng.randn(N, 2)], axis=1)
    logvar = np.concatenate([-8.0 + 0.1 * rng.randn(N, K), np.zeros((N, 2))], axis=1)
    return mean.astype(np.float32), logvar.astype(np.float32)


def rotated_table(seed=0, lat_sizes=GRID):
    """As ideal_table, but the K informative latents are mixed by a random orthogonal matrix and have logvar -3."""
    rng = np.random.RandomState(seed)
    f = _standardised_factors(lat_sizes)
    N, K = f.shape
    rot, _ = np.linalg.qr(rng.randn(K, K))
    mean = np.concatenate([1.5 * f @ rot, 0.01 * rng.randn(N, 2)], axis=1)
    logvar = np.concatenate([np.full((N, K), -3.0), np.zeros((N, 2))], axis=1)
    return mean.astype(np.float32), logvar.astype(np.float32)


# ---- the cases of the GPU test (tests/test_gpu_mass.py); tests/test_mass_host.py measures U_REF on their erfc arguments ---------------
def cases(max_bins=256, block_rows=256, max_chunks=128, lds_doubles=20000):
    """(lat_sizes, D, n_bins, family, S): S None = every row in order, else S row numbers drawn WITH repeats.  The macros of
    include/dvae_mass_hip.h come in as arguments (the callers pass _masslib's mirrors)."""
    small, cap = (4, 3, 2), block_rows * max_chunks
    fit = lds_doubles // max_bins                                    # columns of one workgroup at the most bins
    out = [(small, 3, nb, "broad", None) for nb in (1, 2, 63, 64, 65, 100, 128, 129, max_bins)]      # every wave count, both sides of each
    out += [(GRID, 3, 100, family, None) for family in FAMILIES]
    out += [((3, 2), 1, 2, "far", None), ((3, 2), 1, 1, "broad", 1), ((3, 2), 3, 100, "sharp", 1),
            (small, 17, 129, "edge", None), (GRID, 10, 64, "broad", None), (GRID, 10, 65, "sharp", 1000), (GRID, 17, 4, "wide", 300),
            (GRID, 3, 63, "tiny", 65), (GRID, 1, 100, "edge", 257)]      # a second trip of 64 rows; a second chunk
    # the column split: fit columns in one group, fit + 1 in two
    out += [((40, fit - 40), 1, max_bins, "broad", None), ((40, fit - 39), 1, max_bins, "sharp", None), ((40, fit - 39), 3, max_bins, "wide", 300)]
    # the chunk cap: block_rows * max_chunks rows are max_chunks chunks of block_rows; one row more and the chunks grow
    out += [(small, 1, 4, "broad", S) for S in (cap - 1, cap, cap + 1)]
    return out


_CACHE = {}


def case(lat_sizes, D, n_bins, family, S):
    """Inputs and their fp64 mass table: computed once, shared by the tests, never modified."""
    key = (tuple(lat_sizes), D, n_bins, family, S)
    if key not in _CACHE:
        N = int(np.prod(lat_sizes))
        seed = (1000 * D + 7 * n_bins + N + FAMILIES.index(family)) % (2 ** 31)
        mean, logvar = table(family, N, D, n_bins, seed)
        rows = None if S is None else np.random.RandomState(seed + 1).randint(0, N, S).astype(np.int64)
        mass, n_v = mass_table(mean, logvar, lat_sizes, n_bins, rows=rows)
        _CACHE[key] = dict(mean=mean, logvar=logvar, rows=rows, mass=mass, n_v=n_v, N=N, S=N if S is None else S,
                           cells=np.tile(cell_counts(n_v, lat_sizes, n_bins), (D, 1)))
    return _CACHE[key]


def cell_bound(cells):
    """B of the GPU test: a cell that sums n_v rows is n_v masses, each the difference of two erfc values of at most U_REF ulps
    (values below 1: an ulp is at most 2^-53) formed from a t with the roundings of its exp, product and quotient folded into
    the tails' slope (< 1), the subtraction's own rounding and the addition's -- (2 U_REF + 3) 2^-53 per row."""
    return cells * (2.0 * U_REF + 3.0) * 2.0 ** -53


def erfc_arguments(case_list, limit=20000):
    """A deterministic sample of the arguments math.erfc sees for the tables of `case_list`, both signs."""
    out = []
    for lat_sizes, D, n_bins, family, S in case_list:
        if n_bins < 2:
            continue
        N = int(np.prod(lat_sizes))
        mean, logvar = table(family, min(N, 64), min(D, 3), n_bins, seed=n_bins + D)
        e = edges(n_bins)
        for r in range(mean.shape[0]):
            for d in range(mean.shape[1]):
                out.append(scaled_edges(mean[r, d], logvar[r, d], e))
    t = np.concatenate(out)
    t = np.concatenate([t, -t])
    return t[::max(1, len(t) // limit)]
