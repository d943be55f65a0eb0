"""The InfoVAE / MMD-VAE regulariser (Zhao et al. 2019; WAE-MMD's penalty) restated: fp64 numpy value and ANALYTIC gradients (what
libdvae_mmd_hip.so is compared with), an fp32 numpy form (what a plain fp32 implementation attains: the unit of the GPU tests'
margin), the error bounds of the GPU tests, the tables they run on, and a torch form that composes with oracle.disvae_oracle
under autograd for the whole-step tests.  A plain helper module, like dip_ref.py.

For z, p [B, D], r^2 = |a - b|^2, bandwidth h:  rbf k = exp(-r^2 / h);  imq k = sum_s C_s / (C_s + r^2), C_s = h s, s in SCALES.
  MMD_u = [sum_{i != j} k(z_i, z_j) + sum_{i != j} k(p_i, p_j)] / (B (B - 1)) - 2 sum_{i, j} k(z_i, p_j) / B^2     (B = 1: 0)
  dMMD_u/dz_i = sum_j c_ij (z_i - x_j),  x = [z; p],  c_ij = 2 / (B (B - 1)) k'_ij (z columns, j != i), -2 / B^2 k'_ij (p columns),
  k' = -(2 / h) k (rbf), -2 sum_s C_s / (C_s + r^2)^2 (imq);   dmu = w dMMD_u/dz,  dlv = dmu (z - mu) / 2.

Bounds (u = 2^-53, v = 2^-24, TINY = 2^-126).  The device forms r^2 in fp64 from exact differences, rounds it to fp32 and
evaluates k and c = coefficient * k' in fp32; every sum is fp64.  First order, per pair, with x = r^2 / h:
  rbf   k:  r^2, -1/h and their product are rounded (3 x v), expf is good to one ulp (2 v)             -> (3 x + 4) v k + TINY
        c:  one more product, the coefficient and the product with it                                  -> (3 x + 8) v |c| + |coef| (2 / h) TINY
  imq   a term C / (C + r^2):  C = fl(h) fl(s) (3 v), r^2 (v), the sum (v), v_rcp (one ulp: 2 v), the product (v) = 8 v; the
        seven positive terms are added in fp32 (6 v)                                                   -> 16 v k
        c:  C / (C + r^2)^2 carries the reciprocal twice (13 v), the sum (6 v), coefficient and product (2 v)   -> 24 v |c|
  tol(S)      = sum_pairs [weight v k (+ TINY)] + n u sum_pairs k           (n pairs added in fp64, any order)
  tol(MMD_u)  = (tol(S_zz) + tol(S_pp)) / (B (B - 1)) + 2 tol(S_zp) / B^2 + 8 u (|S_zz| + |S_pp|) / (B (B - 1)) + 16 u |S_zp| / B^2
  tol(dmu_id) = |w| margin sum_j [weight v |c_ij| (+ TINY part)] |z_id - x_jd|  +  v |dmu_id|  +  4 B u |w| sum_j |c_ij| |z_id - x_jd|
  tol(dlv_id) = (tol(dmu_id) - v |dmu_id|) |z_id - mu_id| / 2 + v |dlv_id|
The GPU tests multiply the fp32 part of the gradient bound by the margin max(1, 4 e32), e32 (E32_WORST, pinned by
tests/test_mmd_host.py) the ratio error / tol that fp32_gradients below attains on the same tables, measured on the CPU.
"""
import numpy as np

U = 2.0 ** -53
V = 2.0 ** -24
TINY = 2.0 ** -126
KERNELS = ("rbf", "imq")
TABLES = ("gauss", "regime", "offset", "ties")
SCALES = (0.1, 0.2, 0.5, 1.0, 2.0, 5.0, 10.0)
# worst error / tol of the fp32 restatement (fp32_gradients) over TABLES x KERNELS x the GPU tests' shapes, measured on the CPU
# (test_mmd_host.py measures it again and pins it)
E32_WORST = 0.93         # 0.9348 at ("regime", "rbf", B = 3, D = 128)
MARGIN = max(1.0, 4 * E32_WORST)


def default_bandwidth(D):
    """E r^2 of two standard-normal draws in D dimensions."""
    return 2.0 * D


def table(kind, B, D, seed=0):
    """(z, p, mu) fp32 [B, D]: latent samples, prior draws, posterior means.  gauss: z ~ N(0, I) -- MMD_u is a cancellation of O(1)
    sums.  regime: what a trained encoder emits -- sharp clusters units apart (many RBF terms underflow to 0) beside collapsed
    columns.  offset: z = 30 + 1e-3 noise against p ~ N(0, I) -- |a|^2 + |b|^2 - 2 a.b loses every digit of the z-z distances.
    ties: duplicated rows in z and in p, and z_0 = p_0 -- r^2 = 0 off the diagonal."""
    rng = np.random.default_rng(1000 * seed + 7 * B + D + TABLES.index(kind) * 100003)
    p = rng.standard_normal((B, D))
    if kind == "gauss":
        z = rng.standard_normal((B, D))
        mu = z - 0.3 * rng.standard_normal((B, D))
    elif kind == "regime":
        mu = rng.integers(-3, 4, (B, D)).astype(np.float64) * 1.5
        z = mu + 0.0025 * rng.standard_normal((B, D))                       # exp(logvar / 2) at logvar = -12
        collapsed = np.arange(D) % 3 == 2
        n = int(collapsed.sum())
        mu[:, collapsed] = 1e-3 * rng.standard_normal((B, n))
        z[:, collapsed] = mu[:, collapsed] + rng.standard_normal((B, n))
    elif kind == "offset":
        z = 30.0 + 1e-3 * rng.standard_normal((B, D))
        mu = z - 1e-4 * rng.standard_normal((B, D))
    elif kind == "ties":
        z = rng.standard_normal((B, D))
        z[1::2] = z[0:B - 1:2]
        p[1::2] = p[0:B - 1:2]
        p[0] = z[0]
        if B > 1:
            p[1] = z[0]
        mu = z - 0.3 * rng.standard_normal((B, D))
    else:
        raise ValueError(kind)
    return z.astype(np.float32), p.astype(np.float32), mu.astype(np.float32)


def _r2(a, b, dtype=np.float64):
    """|a_i - b_j|^2 [Na, Nb] from the differences, dimension by dimension."""
    r2 = np.zeros((a.shape[0], b.shape[0]), dtype)
    for d in range(a.shape[1]):
        df = a[:, d, None] - b[None, :, d]
        r2 += df * df
    return r2


def kernel(r2, kind, h):
    """(k, k') of squared distances: d_a k(a, b) = k' (a - b)."""
    one = r2.dtype.type
    if kind == "rbf":
        k = np.exp(-r2 / one(h))
        return k, one(-2.0 / h) * k
    if kind == "imq":
        k, kp = np.zeros_like(r2), np.zeros_like(r2)
        for s in SCALES:
            t = one(h * s) / (one(h * s) + r2)
            k += t
            kp += t / (one(h * s) + r2)
        return k, one(-2.0) * kp
    raise ValueError(kind)


def _weights(r2, kind, h):
    """(value weight, gradient weight) of the module docstring's per-pair bounds, in units of v."""
    if kind == "rbf":
        x = r2 / h
        return 3 * x + 4, 3 * x + 8
    return np.full_like(r2, 16.0), np.full_like(r2, 24.0)


def _coefficients(B):
    b = float(B)
    return (2.0 / (b * (b - 1.0)) if B > 1 else 0.0), -2.0 / (b * b)


def mmd(z, p, kind, h, w=1.0, mu=None, bounds=True):
    """fp64 -> dict(mmd, wmmd, S_zz, S_pp, S_zp, dz = dMMD_u/dz, dmu = w dz, dlv (None without mu), and, with bounds, what
    tolerances() needs)."""
    z64, p64 = np.asarray(z, np.float64), np.asarray(p, np.float64)
    B, D = z64.shape
    x0 = z64[0].copy()                                                       # a shift: distances and gradients do not move
    zc, pc = z64 - x0, p64 - x0
    X = np.concatenate([zc, pc])
    r2 = _r2(zc, X)                                                          # [B, 2 B]
    r2pp = _r2(pc, pc)
    k, kp = kernel(r2, kind, h)
    kpp, _ = kernel(r2pp, kind, h)
    off = ~np.eye(B, dtype=bool)
    S_zz, S_zp, S_pp = (k[:, :B] * off).sum(), k[:, B:].sum(), (kpp * off).sum()
    czz, czp = _coefficients(B)
    val = (S_zz + S_pp) * czz / 2.0 + czp * S_zp if B > 1 else 0.0
    c = np.concatenate([czz * kp[:, :B] * off, czp * kp[:, B:]], axis=1)
    if B == 1:
        c[:] = 0.0
    out = dict(B=B, D=D, kind=kind, h=h, w=w, mmd=val, wmmd=w * val, S_zz=S_zz, S_pp=S_pp, S_zp=S_zp)
    wv, wg = _weights(r2, kind, h)
    flush = TINY if kind == "rbf" else 0.0
    cabs = np.abs(c)
    cerr = cabs * wg * V
    if kind == "rbf" and B > 1:
        cerr = cerr + np.concatenate([np.full((B, B), czz) * off, np.full((B, B), -czp)], axis=1) * (2.0 / h) * TINY
    dz, gabs, gerr = np.zeros((B, D)), np.zeros((B, D)), np.zeros((B, D))
    for d in range(D):
        diff = zc[:, d, None] - X[None, :, d]
        dz[:, d] = (c * diff).sum(axis=1)
        if bounds:
            ad = np.abs(diff)
            gabs[:, d] = (cabs * ad).sum(axis=1)
            gerr[:, d] = (cerr * ad).sum(axis=1)
    out.update(dz=dz, dmu=w * dz, dlv=None, half=None)
    if mu is not None:
        out["half"] = 0.5 * (z64 - np.asarray(mu, np.float64))
        out["dlv"] = out["dmu"] * out["half"]
    if bounds:
        wpp, _ = _weights(r2pp, kind, h)
        n = B * B
        out.update(gabs=gabs, gerr=gerr,
                   tS_zz=((wv[:, :B] * V * k[:, :B] + flush) * off).sum() + n * U * S_zz,
                   tS_zp=(wv[:, B:] * V * k[:, B:] + flush).sum() + n * U * S_zp,
                   tS_pp=((wpp * V * kpp + flush) * off).sum() + n * U * S_pp)
    return out


def tolerances(ref, margin=1.0):
    """The module docstring's bounds for one mmd() result -> dict(S_zz, S_pp, S_zp, mmd, wmmd, dmu, dlv)."""
    B, w = ref["B"], abs(ref["w"])
    czz, czp = _coefficients(B)
    tm = 0.0
    if B > 1:
        tm = (ref["tS_zz"] + ref["tS_pp"]) * czz / 2 - czp * ref["tS_zp"] + 8 * U * (ref["S_zz"] + ref["S_pp"]) * czz / 2 \
            - 8 * U * czp * ref["S_zp"]
    tg = w * margin * ref["gerr"] + 4 * B * U * w * ref["gabs"]
    tdmu = tg + V * np.abs(ref["dmu"])
    tdlv = None if ref["dlv"] is None else tg * np.abs(ref["half"]) + V * np.abs(ref["dlv"])
    return dict(S_zz=ref["tS_zz"], S_pp=ref["tS_pp"], S_zp=ref["tS_zp"], mmd=tm, wmmd=w * tm + 2 * U * abs(ref["wmmd"]), dmu=tdmu,
                dlv=tdlv)


def mmd_literal(z, p, kind, h):
    """MMD_u and dMMD_u/dz by the literal double loop over pairs (small B only)."""
    z, p = np.asarray(z, np.float64), np.asarray(p, np.float64)
    B, D = z.shape

    def kk(a, b):
        r2 = np.array(((a - b) ** 2).sum())
        k, kp = kernel(r2, kind, h)
        return float(k), float(kp) * (a - b)
    if B == 1:
        return 0.0, np.zeros((B, D))
    szz = spp = szp = 0.0
    g = np.zeros((B, D))
    for i in range(B):
        for j in range(B):
            if i != j:
                k, dk = kk(z[i], z[j])
                szz += k
                g[i] += 2.0 / (B * (B - 1)) * dk
                spp += kk(p[i], p[j])[0]
            k, dk = kk(z[i], p[j])
            szp += k
            g[i] -= 2.0 / (B * B) * dk
    return (szz + spp) / (B * (B - 1)) - 2.0 * szp / (B * B), g


def mmd_norm_expansion(z, p, kind, h, dtype=np.float32):
    """S_zz with r^2 = |a|^2 + |b|^2 - 2 a.b in `dtype`: the form the library must never use (it fails the offset table)."""
    z = np.asarray(z, dtype)
    n = (z * z).sum(axis=1)
    r2 = np.maximum(n[:, None] + n[None, :] - dtype(2) * (z @ z.T), dtype(0))
    k, _ = kernel(r2, kind, h)
    return float((k.astype(np.float64) * ~np.eye(z.shape[0], dtype=bool)).sum())


def fp32_gradients(z, p, kind, h, w=1.0, mu=None):
    """The whole computation in fp32 -> (dmu, dlv): differences, r^2, k', the coefficients, the products and their sums over the
    2 B columns are fp32 operations on the fp32 inputs.  This is the unit of the fp32 part of the gradient bound."""
    f = np.float32
    z, p = np.asarray(z, f), np.asarray(p, f)
    B, D = z.shape
    X = np.concatenate([z, p])
    _, kp = kernel(_r2(z, X, f), kind, h)
    czz, czp = _coefficients(B)
    off = ~np.eye(B, dtype=bool)
    c = np.concatenate([f(czz) * kp[:, :B] * off, f(czp) * kp[:, B:]], axis=1).astype(f)
    if B == 1:
        c[:] = 0
    dz = np.zeros((B, D), f)
    for d in range(D):
        dz[:, d] = (c * (z[:, d, None] - X[None, :, d])).sum(axis=1, dtype=f)
    dmu = (f(w) * dz).astype(f)
    dlv = None if mu is None else (dmu * (f(0.5) * (z - np.asarray(mu, f)))).astype(f)
    return dmu, dlv


def e32(kind_table, B, D, kind, w=1.0):
    """error / tol (margin 1) that fp32_gradients attains on one table: the worst over dmu and dlv."""
    z, p, mu = table(kind_table, B, D)
    h = default_bandwidth(D)
    ref = mmd(z, p, kind, h, w, mu)
    tol = tolerances(ref)
    dmu, dlv = fp32_gradients(z, p, kind, h, w, mu)
    return max(float((np.abs(dmu - ref["dmu"]) / (tol["dmu"] + 1e-300)).max()),
               float((np.abs(dlv - ref["dlv"]) / (tol["dlv"] + 1e-300)).max()))


# ---- torch, for autograd and the whole-step tests ---------------------------------------------------------------------------------
def regulariser_torch(z, p, kind, h):
    """MMD_u(z, p) as a differentiable torch scalar in z's dtype."""
    import torch
    B = z.shape[0]
    if B == 1:
        return z.sum() * 0.0

    def gram(a, b):
        r2 = ((a[:, None, :] - b[None, :, :]) ** 2).sum(dim=2)
        if kind == "rbf":
            return torch.exp(-r2 / h)
        return sum((h * s) / (h * s + r2) for s in SCALES)
    off = 1.0 - torch.eye(B, dtype=z.dtype, device=z.device)
    return ((gram(z, z) * off).sum() + (gram(p, p) * off).sum()) / (B * (B - 1)) - 2.0 * gram(z, p).sum() / (B * B)


def mmd_iteration_grads(hp, state, params, data, eps, prior):
    """oracle.disvae_oracle.train_iteration_grads for "infovae": vae_forward + single_optimizer_loss("betaH", beta = 1 - alpha) +
    (alpha + lam - 1) MMD_u(z, prior) -> (loss, logs, grads, outs); logs in the order InfoVaeLoss stores them (recon_loss, kl_loss,
    kl_loss_i, mmd_loss, loss)."""
    from collections import OrderedDict

    import torch
    from oracle import disvae_oracle as O
    alpha, lam = hp.get("info_alpha", 0.0), hp.get("info_lambda", 1000.0)
    kind, h = hp.get("mmd_kernel", "imq"), hp.get("mmd_bandwidth")
    recon, (mu, logvar), z = O.vae_forward(params, data, eps)
    h = default_bandwidth(z.shape[1]) if h is None else h
    base, logs, _ = O.single_optimizer_loss("betaH", dict(hp, betaH_B=1.0 - alpha), state, data, recon, mu, logvar, z, True)
    R = (alpha + lam - 1.0) * regulariser_torch(z, prior.to(z.dtype), kind, h)
    loss = base + R
    out_logs = OrderedDict((k, v.detach()) for k, v in logs.items() if k != "loss")
    out_logs["mmd_loss"] = R.detach()
    out_logs["loss"] = loss.detach()
    grads = torch.autograd.grad(loss, list(params.values()), allow_unused=True)
    grads = OrderedDict((k, g) for k, g in zip(params.keys(), grads))
    outs = dict(recon=recon.detach(), mu=mu.detach(), logvar=logvar.detach(), z=z.detach())
    return loss.detach(), out_logs, grads, outs
