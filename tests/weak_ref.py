"""fp64 restatement of the adaptive group posterior of Ada-GVAE / Ada-ML-VAE (include/dvae_weak_hip.h; Locatello et al. 2020) for
the tests: numpy (values, mask, band, first-order fp32 bounds), torch (differentiable, the mask an input), the tables the kernels
are run on, and the oracle of a whole pair step.  A plain helper module, like dip_ref.py.

A batch has 2 P rows, rows i and P + i are pair i (a = row i, b = row P + i):
    delta = exp(lv_a - lv_b) + (mu_b - mu_a)^2 exp(-lv_b) - 1 + (lv_b - lv_a)        four terms T1 .. T4
    tau   = (max_d delta + min_d delta) / 2;  shared: delta < tau, strictly
    gvae  m = (mu_a + mu_b) / 2,               lv~ = max(lv) + log1p(exp(-|t|)) - log 2,   t = lv_b - lv_a
    mlvae m = w mu_a + (1 - w) mu_b, w = sigmoid(t),  lv~ = log 2 + min(lv) - log1p(exp(-|t|))

THE BAND.  An entry whose |delta - tau| <= BAND * (S_d + S_max + S_min), S the sum of the absolute values of the four terms of
that dimension / of the arg-max / of the arg-min dimension, may be masked either way by an fp32 evaluation; outside it the fp32
mask must be the fp64 one bit for bit.  BAND = 1e-5 is ~17 times the fp32 error bound of one delta (about 10 u S, u = 2^-24).

THE BOUNDS (derived in DESIGN.md section 2; u = 2^-24, first order, margin 1; the GPU tests allow MARGIN = 4 times them).  With
x = lv_a - lv_b, e = exp(-|t|), sp = log1p(e), wa = sigmoid(t), wb = sigmoid(-t), an exp / log1p of 2 u, a correctly rounded
division and TINY = 2^-126 for results that underflow:
    delta    u ((|x| + 3) T1 + 6 T2 + |T4| + 3 S)
    gvae     m: u (|mu_a| + |mu_b|) / 2        lv~: u (e (|t| + 2) + 2 sp + |max + sp| + |lv~| + 0.7)
    mlvae    m: u (|wa mu_a| (wb (|t| + 2) + 3) + |wb mu_b| (wa (|t| + 2) + 3) + |m|)
             lv~: u (0.7 + |log 2 + min| + e (|t| + 2) + 2 sp + |lv~|)
    backward, Ga = |g_a| + |g_b| of the mu~ gradients, Gl of the lv~ gradients:
    gvae     dmu: u Ga / 2                      dlv_a: u Gl wb (wa (|t| + 2) + 4)   (dlv_b: wa <-> wb)
    mlvae    dmu_a: u Ga wa (wb (|t| + 2) + 4)  (dmu_b: wa <-> wb);  c = Ga wa wb |mu_a - mu_b|,  E_c = u c (|t| + 11)
             dlv_a: u Gl wa (wb (|t| + 2) + 4) + E_c + u (Gl wa + c)                (dlv_b: wa <-> wb)
Elements of a dimension that is not shared are copies (forward) or untouched (backward): bit for bit.
"""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126
BAND = 1e-5
MARGIN = 4.0
LOG2 = float(np.log(2.0))
KINDS = ("gvae", "mlvae")
FAMILIES = ("gauss", "regime")
# (P, D) of the CPU band test and of the GPU kernel tests
HOST_SIZES = ((1, 2), (3, 10), (64, 10), (257, 16), (33, 20), (5, 64))
GPU_SIZES = ((1, 1), (1, 2), (3, 10), (64, 10), (65, 16), (257, 17), (33, 20), (5, 64), (1024, 10))


# ---- the operator, numpy ------------------------------------------------------------------------------------------------------------
def split(mu, lv):
    """[2 P, D] -> (mu_a, lv_a, mu_b, lv_b), each [P, D], in the dtype given."""
    P = mu.shape[0] // 2
    assert mu.shape[0] == 2 * P and mu.shape == lv.shape
    return mu[:P], lv[:P], mu[P:], lv[P:]


def delta_terms(mu, lv, dtype=np.float64):
    """The four terms of delta, [4, P, D], evaluated in `dtype` in the order the header writes them."""
    ma, la, mb, lb = (np.asarray(v, dtype=dtype) for v in split(mu, lv))
    one = dtype(1.0)
    with np.errstate(over="ignore", invalid="ignore"):
        t1 = np.exp(la - lb)
        dm = mb - ma
        t2 = dm * dm * np.exp(-lb)
        return np.stack([t1, t2, np.full_like(t1, -one), lb - la])


def delta_of(terms):
    with np.errstate(invalid="ignore"):
        return ((terms[0] + terms[1]) + terms[2]) + terms[3]


def mask_of(delta):
    """(tau [P], shared bool [P, D]); min / max skip a NaN (fmin / fmax), a NaN compares false."""
    with np.errstate(invalid="ignore", over="ignore"):
        half = delta.dtype.type(0.5)
        tau = half * np.fmax.reduce(delta, axis=1) + half * np.fmin.reduce(delta, axis=1)
        return tau, delta < tau[:, None]


def band_of(mu, lv):
    """bool [P, D]: the entries an fp32 evaluation may mask either way."""
    terms = delta_terms(mu, lv)
    delta = delta_of(terms)
    tau, _ = mask_of(delta)
    S = np.abs(terms).sum(axis=0)
    rows = np.arange(delta.shape[0])
    with np.errstate(invalid="ignore"):
        hi, lo = np.nanargmax(delta, axis=1), np.nanargmin(delta, axis=1)
        width = BAND * (S + (S[rows, hi] + S[rows, lo])[:, None])
        return np.abs(delta - tau[:, None]) <= width


def mask_fp32(mu, lv):
    """The mask of a numpy float32 evaluation in the device's operation order."""
    return mask_of(delta_of(delta_terms(mu, lv, np.float32)))[1]


def _pieces(ma, la, mb, lb):
    t = lb - la
    e = np.exp(-np.abs(t))
    sp = np.log1p(e)
    with np.errstate(over="ignore"):
        wa, wb = 1.0 / (1.0 + np.exp(-t)), 1.0 / (1.0 + np.exp(t))
    return t, e, sp, wa, wb


def aggregate(mu, lv, kind, shared=None):
    """fp64 -> dict(mu, lv [2 P, D] aggregated; shared bool [P, D] (the one given, else the restatement's own); delta, tau;
    m, lvt [P, D]: the aggregated values of EVERY dimension, shared or not)."""
    assert kind in KINDS
    mu64, lv64 = np.asarray(mu, dtype=np.float64), np.asarray(lv, dtype=np.float64)
    ma, la, mb, lb = split(mu64, lv64)
    delta = delta_of(delta_terms(mu64, lv64))
    tau, own = mask_of(delta)
    sh = own if shared is None else np.asarray(shared, dtype=bool)
    t, e, sp, wa, wb = _pieces(ma, la, mb, lb)
    if kind == "gvae":
        m = 0.5 * (ma + mb)
        lvt = np.maximum(la, lb) + sp - LOG2
    else:
        m = wa * ma + wb * mb
        lvt = LOG2 + np.minimum(la, lb) - sp
    out_mu = np.concatenate([np.where(sh, m, ma), np.where(sh, m, mb)])
    out_lv = np.concatenate([np.where(sh, lvt, la), np.where(sh, lvt, lb)])
    return dict(mu=out_mu, lv=out_lv, shared=sh, own=own, delta=delta, tau=tau, m=m, lvt=lvt)


def mlvae_literal(mu, lv):
    """The product of experts as disentanglement_lib's MLVae writes it: var~ = 2 v_a v_b / (v_a + v_b),
    m = (mu_a / v_a + mu_b / v_b) var~ / 2 -> (m, log var~)."""
    ma, la, mb, lb = split(np.asarray(mu, dtype=np.float64), np.asarray(lv, dtype=np.float64))
    va, vb = np.exp(la), np.exp(lb)
    var = 2.0 * va * vb / (va + vb)
    return (ma / va + mb / vb) * var / 2.0, np.log(var)


def bits_of(shared):
    """bool [P, D] -> the mask words, uint64 [P]."""
    sh = np.asarray(shared, dtype=bool)
    w = np.zeros(sh.shape[0], dtype=np.uint64)
    for d in range(sh.shape[1]):
        w |= sh[:, d].astype(np.uint64) << np.uint64(d)
    return w


def unbits(words, D):
    """int64 / uint64 [P] -> bool [P, D]."""
    w = np.asarray(words).astype(np.int64).view(np.uint64)
    return np.stack([(w >> np.uint64(d)) & np.uint64(1) for d in range(D)], axis=1).astype(bool)


def interleave(mu, lv):
    """[B, D] x 2 -> the [B, 2 D] layout of mu_logvar_gen."""
    return np.stack([mu, lv], axis=-1).reshape(mu.shape[0], -1)


# ---- first-order fp32 bounds (margin 1) ------------------------------------------------------------------------------------------------
def forward_bounds(mu, lv, kind):
    """dict(delta [P, D], m [P, D], lvt [P, D]): |device - fp64| allowed at margin 1 for delta and for a SHARED element."""
    mu64, lv64 = np.asarray(mu, dtype=np.float64), np.asarray(lv, dtype=np.float64)
    ma, la, mb, lb = split(mu64, lv64)
    T = np.abs(delta_terms(mu64, lv64))
    S = T.sum(axis=0)
    e_delta = U * ((np.abs(la - lb) + 3) * T[0] + 6 * T[1] + T[3] + 3 * S) + TINY
    t, e, sp, wa, wb = _pieces(ma, la, mb, lb)
    at = np.abs(t)
    if kind == "gvae":
        lvt = np.maximum(la, lb) + sp - LOG2
        e_m = U * 0.5 * (np.abs(ma) + np.abs(mb)) + TINY
        e_lv = U * (e * (at + 2) + 2 * sp + np.abs(np.maximum(la, lb) + sp) + np.abs(lvt) + 0.7)
    else:
        lvt = LOG2 + np.minimum(la, lb) - sp
        m = wa * ma + wb * mb
        e_m = U * (np.abs(wa * ma) * (wb * (at + 2) + 3) + np.abs(wb * mb) * (wa * (at + 2) + 3) + np.abs(m)) + TINY
        e_lv = U * (0.7 + np.abs(LOG2 + np.minimum(la, lb)) + e * (at + 2) + 2 * sp + np.abs(lvt))
    return dict(delta=e_delta, m=e_m, lvt=e_lv)


def backward_bounds(mu, lv, gmu, glv, kind):
    """(e_dmu [2 P, D], e_dlv [2 P, D]): |device - fp64| allowed at margin 1 for the gradient of a SHARED element."""
    ma, la, mb, lb = split(np.asarray(mu, dtype=np.float64), np.asarray(lv, dtype=np.float64))
    P = ma.shape[0]
    g = np.abs(np.asarray(gmu, dtype=np.float64))
    h = np.abs(np.asarray(glv, dtype=np.float64))
    Ga, Gl = g[:P] + g[P:], h[:P] + h[P:]
    t, e, sp, wa, wb = _pieces(ma, la, mb, lb)
    at = np.abs(t)
    ra, rb = wb * (at + 2) + 4, wa * (at + 2) + 4                     # relative error (in u) of a product with wa / with wb
    if kind == "gvae":
        e_mu = U * 0.5 * Ga + TINY
        return np.concatenate([e_mu, e_mu]), np.concatenate([U * Gl * wb * rb, U * Gl * wa * ra]) + TINY
    c = Ga * wa * wb * np.abs(ma - mb)
    e_c = U * c * (at + 11)
    e_mu = np.concatenate([U * Ga * wa * ra, U * Ga * wb * rb]) + TINY
    e_lv = np.concatenate([U * Gl * wa * ra + e_c + U * (Gl * wa + c), U * Gl * wb * rb + e_c + U * (Gl * wb + c)]) + TINY
    return e_mu, e_lv


# ---- torch: differentiable, the mask an input ----------------------------------------------------------------------------------------
def aggregate_torch(mu, lv, kind, shared):
    """mu, lv torch [2 P, D] (any float dtype, may require grad), shared bool [P, D] (a constant) -> (mu~, lv~) [2 P, D]."""
    import math

    import torch
    assert kind in KINDS
    P = mu.shape[0] // 2
    ma, mb, la, lb = mu[:P], mu[P:], lv[:P], lv[P:]
    sh = torch.as_tensor(np.asarray(shared, dtype=bool)) if not torch.is_tensor(shared) else shared.bool()
    t = lb - la
    sp = torch.log1p(torch.exp(-t.abs()))
    if kind == "gvae":
        m = 0.5 * (ma + mb)
        lvt = torch.maximum(la, lb) + sp - math.log(2.0)
    else:
        # not torch.sigmoid: its backward is s (1 - s), and 1 - s is 0 in fp64 from |t| = 37 on -- d/dt of 1 / (1 + exp(-t)) has no
        # such cancellation
        m = ma / (1.0 + torch.exp(-t)) + mb / (1.0 + torch.exp(t))
        lvt = math.log(2.0) + torch.minimum(la, lb) - sp
    return (torch.cat([torch.where(sh, m, ma), torch.where(sh, m, mb)]),
            torch.cat([torch.where(sh, lvt, la), torch.where(sh, lvt, lb)]))


def own_mask_torch(mu, lv):
    """The restatement's own mask of torch tensors (detached, fp64) -> bool ndarray [P, D]."""
    return aggregate(mu.detach().cpu().double().numpy(), lv.detach().cpu().double().numpy(), "gvae")["own"]


# ---- tables -----------------------------------------------------------------------------------------------------------------------------
def table(family, P, D, seed=0):
    """(mu, lv) float32 [2 P, D].
    gauss    mu ~ N(0, 1), lv ~ U(-6, 0), every row independent;
    regime   a trained model: min(5, D) sharp dimensions with lv -9 / -12 at integer means in [-3, 3], the others collapsed
             (mu = 0, lv = 0), 1e-2 Gaussian jitter on every entry of both rows, and per pair ONE sharp dimension whose mean is
             moved by +-1 / +-2 in the partner."""
    rng = np.random.RandomState(1000 * seed + 17 * P + D + (0 if family == "gauss" else 500000))
    if family == "gauss":
        return rng.randn(2 * P, D).astype(np.float32), rng.uniform(-6.0, 0.0, (2 * P, D)).astype(np.float32)
    assert family == "regime"
    ns = min(5, D)
    mu, lv = np.zeros((P, D)), np.zeros((P, D))
    mu[:, :ns] = rng.randint(-3, 4, (P, ns))
    lv[:, :ns] = np.where(np.arange(ns) % 2 == 0, -9.0, -12.0)
    mu_b = mu.copy()
    moved = rng.randint(0, ns, P)
    mu_b[np.arange(P), moved] += rng.choice([-2.0, -1.0, 1.0, 2.0], P)
    mu2, lv2 = np.concatenate([mu, mu_b]), np.concatenate([lv, lv])
    return ((mu2 + 1e-2 * rng.randn(2 * P, D)).astype(np.float32), (lv2 + 1e-2 * rng.randn(2 * P, D)).astype(np.float32))


def edge_table(D):
    """(mu, lv, expected) float32 [2 * 6, D] and the mask words that ANY correct evaluation gives for pairs 0 .. 2 (None for the
    others: those go through the band):
      0  identical rows: every delta is 0, nothing is shared;
      1  every dimension holds the same numbers: all deltas tie, nothing is shared;
      2  two groups of tied deltas (D >= 2): dimensions d < ceil(D / 2) tie below tau and are shared, the others tie above it;
      3  lv differences of +40 and -40 on alternating dimensions;
      4  lv_a = -20 against lv_b = +4 on dimension 0, Gaussian elsewhere;
      5  lv_a = +4 against lv_b = -20 on the last dimension, Gaussian elsewhere."""
    rng = np.random.RandomState(77 + D)
    P = 6
    mu = rng.randn(2 * P, D).astype(np.float32)
    lv = rng.uniform(-6.0, 0.0, (2 * P, D)).astype(np.float32)
    mu[P + 0], lv[P + 0] = mu[0], lv[0]
    mu[1], lv[1], mu[P + 1], lv[P + 1] = 0.25, -1.5, -0.5, -2.0
    half = (D + 1) // 2
    mu[2], lv[2], mu[P + 2], lv[P + 2] = 0.5, -3.0, 0.5, -3.0
    mu[2, :half], mu[P + 2, :half] = 1.0, 1.125                          # a small delta, tied
    mu[2, half:], mu[P + 2, half:] = 1.0, 3.0                            # a large one, tied
    sign = np.where(np.arange(D) % 2 == 0, 1.0, -1.0).astype(np.float32)
    lv[3], lv[P + 3] = 20.0 * sign, -20.0 * sign
    lv[4, 0], lv[P + 4, 0] = -20.0, 4.0
    lv[5, D - 1], lv[P + 5, D - 1] = 4.0, -20.0
    two = bits_of((np.arange(D) < half)[None, :])[0] if D >= 2 else np.uint64(0)
    return mu, lv, [np.uint64(0), np.uint64(0), two, None, None, None]


# ---- the oracle of a whole pair step ----------------------------------------------------------------------------------------------------
def weak_iteration_grads(aggregation, hp, state, params, data, eps, shared=None, is_train=True):
    """oracle.disvae_oracle.train_iteration_grads for "adagvae" / "adamlvae" (aggregation "gvae" / "mlvae"): encoder -> adaptive
    group posterior -> reparameterisation -> decoder -> rec + anneal * beta * KL(q~ || N(0, I)), both batch means over the 2 P
    rows -> (loss, logs, grads, outs).  shared: bool [P, D], the mask to aggregate under (a constant for the gradient); None: the
    restatement's own.  logs in the order WeakVaeLoss stores them (recon_loss, kl_loss, kl_loss_i, shared_dims, loss); outs also
    holds the un-aggregated posterior (mu0, logvar0) and the mask used.  eps None: z = m~ (evaluation)."""
    from collections import OrderedDict

    import torch
    from oracle import disvae_oracle as O
    mu0, logvar0 = O.encoder_forward(params, data)
    if shared is None:
        shared = own_mask_torch(mu0, logvar0)
    shared = np.asarray(shared, dtype=bool)
    mu, logvar = aggregate_torch(mu0, logvar0, aggregation, shared)
    z = O.reparameterize(mu, logvar, eps)
    recon = O.decoder_forward(params, z)
    if is_train:
        state.n_train_steps += 1
    rec = O.reconstruction_loss(data, recon, state.rec_dist)
    kl, kl_i = O.kl_normal_loss(mu, logvar)
    anneal = O.linear_annealing(0, 1, state.n_train_steps, state.steps_anneal) if is_train else 1
    loss = rec + anneal * (hp.get("weak_beta", 1) * kl)
    logs = OrderedDict(recon_loss=rec.detach(), kl_loss=kl.detach())
    for i in range(kl_i.numel()):
        logs["kl_loss_%d" % i] = kl_i[i].detach()
    logs["shared_dims"] = torch.tensor(float(shared.sum(axis=1).mean()), dtype=torch.float64)
    logs["loss"] = loss.detach()
    grads = None
    if is_train:
        grads = torch.autograd.grad(loss, list(params.values()), allow_unused=True)
        grads = OrderedDict((k, g) for k, g in zip(params.keys(), grads))
    outs = dict(recon=recon.detach(), mu=mu.detach(), logvar=logvar.detach(), z=z.detach(), mu0=mu0.detach(),
                logvar0=logvar0.detach(), shared=shared)
    return loss.detach(), logs, grads, outs
