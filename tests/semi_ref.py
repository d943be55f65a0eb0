"""The supervised regulariser of S2-beta-VAE (Locatello et al. 2020, "Disentangling Factors of Variation Using Few Labels";
disentanglement_lib's semi_supervised_vae.py) restated: the label arithmetic, fp64 numpy values and ANALYTIC gradients of the
three forms (what libdvae_semi_hip.so is compared with), an fp32 numpy form of the gradients (what a plain fp32 implementation
attains: the unit of the GPU tests' margin), the error bounds of the GPU tests, the tables and labelling patterns they run on,
and a torch form that composes with oracle.disvae_oracle under autograd for the whole-step tests.  A plain helper module, like
dip_ref.py.

The data set enumerates lat_sizes by row number in row-major order; rows[i] < 0: image i is unlabelled; L the labelled rows,
n_lab = |L|; factor factors[k] is tied to latent k; v_ik = (rows[i] // stride_k) % size_k, y_ik = v_ik / size_k.
  xent  R = sum_{i in L, k<K} max(x, 0) - x y_ik + log1p(exp(-|x|)), x = mu_ik;   dR/dmu_ik = sigmoid(mu_ik) - y_ik
  l2    R = sum_{i in L, k<K} (mu_ik - y_ik)^2;                                    dR/dmu_ik = 2 (mu_ik - y_ik)
  cov   R = sum_{d != k} C_dk^2, C [D, K] the biased cross-covariance of mu and v over L;  G = dR/dC (0 where d = k, else 2 C);
        dR/dmu_id = (1 / n_lab) sum_k G_dk (v_ik - mean v_k)
"mean" divides xent and l2 (value and gradient) by n_lab.  n_lab = 0: everything is 0.  The gradient returned is w dR/dmu.

Bounds (u = 2^-53, v = 2^-24).  The device adds fp64 terms in a fixed order, the covariance around the first labelled row 0:
  tol(R)      = 8 (n_lab K) u sum |terms|                       xent: |terms| = max(x, 0) + |x y| + log1p(exp(-|x|)); l2: the term
  tol(C_dk)   = 8 n_lab u sqrt(m2_d s2_k),   m2_d = mean_L (mu_id - mu_0d)^2, s2_k = mean_L (v_ik - v_0k)^2
-- the bound the project already uses for fp64 covariances (dip_ref, unsup_ref.tol_cov), the worst case of an n-term sum by
Cauchy-Schwarz --
  tol(R cov)  = sum_dk |G_dk| tol(C_dk) + 8 D K u |R|           (first order in the error of C, plus the fp64 sum of D K terms)
  tol(dmu_id) = GRAD_ULPS v M_id  +  (w / n_lab) sum_k 2 tol(C_dk) |v_ik - mean v_k|   (the second part: cov only)
with M the sum of the magnitudes the gradient is made of: w s (sigmoid(x) + y) for xent, 2 w s (|x| + y) for l2 (s = 1 or
1 / n_lab), (w / n_lab) sum_k |G_dk| |v_ik - mean v_k| for cov.  GRAD_ULPS = 4 as in dip_ref.  Every gradient bound also carries
TINY = 2^-126, the fp32 underflow threshold: sigmoid(-100) = 4e-44 is a denormal that fp32 holds with no relative accuracy.  The GPU tests multiply the fp32
part by the margin max(1, 4 e32), e32 (E32_WORST, pinned by tests/test_semi_host.py) the ratio error / tol that fp32_gradients
below attains on the same tables, measured on the CPU -- never from the device's output.
"""
import numpy as np

U = 2.0 ** -53
V = 2.0 ** -24
GRAD_ULPS = 4
TINY = 2.0 ** -126          # the smallest normal fp32: below it a stored gradient has no relative accuracy (sigmoid(-100) = 4e-44)
KINDS =("xent", "l2", "cov")
REDUCTIONS = ("sum", "mean")
TABLES = ("gauss", "offset", "regime", "far40", "far100")
PATTERNS = ("all", "none", "alternating", "last", "second_half")
DSPRITES = (1, 3, 6, 40, 32, 32)
ONE_VALUE = (4, 1, 5, 3)                  # a size-1 factor in the middle: its value is always 0
# worst error / tol of the fp32 restatement of the gradients (fp32_gradients) over the GPU tests' cases, measured on the CPU
# (test_semi_host.py measures it again and pins it)
E32_WORST = 1.06         # 1.060 at ("xent", "gauss", ONE_VALUE, n = 63, D = 64, "all", "mean")
MARGIN = max(1.0, 4 * E32_WORST)


# ---- labels -------------------------------------------------------------------------------------------------------------------
def strides_of(lat_sizes):
    sizes = [int(s) for s in lat_sizes]
    return [int(np.prod(sizes[j + 1:], dtype=np.int64)) for j in range(len(sizes))]


def default_factors(lat_sizes):
    return [j for j, s in enumerate(lat_sizes) if int(s) >= 2]


def values(rows, lat_sizes, factors):
    """int64 [n, K]: the value index of every chosen factor of every row (garbage where rows < 0: mask with labelled())."""
    rows = np.asarray(rows, np.int64)
    st = strides_of(lat_sizes)
    return np.stack([(rows // st[j]) % int(lat_sizes[j]) for j in factors], axis=1)


def labelled(rows):
    return np.asarray(rows, np.int64) >= 0


def rows_for(n, lat_sizes, pattern, seed=0):
    """int64 [n] row numbers under a labelling pattern; an unlabelled row holds SOME negative number (-1, or -1 - its row)."""
    rng = np.random.default_rng(77 * seed + 13 * n + len(lat_sizes) + PATTERNS.index(pattern) * 1009)
    total = int(np.prod([int(s) for s in lat_sizes], dtype=np.int64))
    r = rng.integers(0, total, n).astype(np.int64)
    on = {"all": np.ones(n, bool), "none": np.zeros(n, bool), "alternating": np.arange(n) % 2 == 1,
          "last": np.arange(n) == n - 1, "second_half": np.arange(n) >= n // 2}[pattern]
    neg = np.where(np.arange(n) % 3 == 0, -1, -1 - r)
    return np.where(on, r, neg).astype(np.int64)


def table(kind, n, D, seed=0):
    """mu fp32 [n, D].  gauss: N(0, 1).  offset: 30 + 1e-3 noise -- a raw-moment fp32 sum loses every digit of the covariance
    there.  regime: the means of latent_regimes.family("trained"): cluster centres units apart beside collapsed columns.
    far40 / far100: means at +-40 / +-100 (random signs), where a naive sigmoid or BCE overflows."""
    rng = np.random.default_rng(1000 * seed + 7 * n + D + TABLES.index(kind) * 100003)
    if kind == "gauss":
        mu = rng.standard_normal((n, D))
    elif kind == "offset":
        mu = 30.0 + 1e-3 * rng.standard_normal((n, D))
    elif kind == "regime":
        import latent_regimes
        mu = latent_regimes.family("trained", n, D, seed=4000 + n + 31 * D + seed)[1].numpy().astype(np.float64)
    elif kind in ("far40", "far100"):
        mu = float(kind[3:]) * rng.choice([-1.0, 1.0], (n, D)) + 1e-2 * rng.standard_normal((n, D))
    else:
        raise ValueError(kind)
    return mu.astype(np.float32)


# ---- fp64 -------------------------------------------------------------------------------------------------------------------------
def sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def bce_with_logits(x, y):
    return np.maximum(x, 0.0) - x * y + np.log1p(np.exp(-np.abs(x)))


def regulariser(mu, rows, lat_sizes, kind, reduction="sum", w=1.0, factors=None):
    """fp64 -> dict(R, n_lab, C [D, K] (zeros for xent / l2), G, dmu = w dR/dmu, and what the bounds need)."""
    mu64 = np.asarray(mu, np.float64)
    n, D = mu64.shape
    factors = default_factors(lat_sizes) if factors is None else list(factors)
    K = len(factors)
    assert 1 <= K <= D
    on = labelled(rows)
    n_lab = int(on.sum())
    v = values(np.where(on, rows, 0), lat_sizes, factors).astype(np.float64)
    sizes = np.array([int(lat_sizes[j]) for j in factors], np.float64)
    y = v / sizes
    s = 1.0 / n_lab if (reduction == "mean" and n_lab) else 1.0
    C, G = np.zeros((D, K)), np.zeros((D, K))
    dmu, mag, prop = np.zeros((n, D)), np.zeros((n, D)), np.zeros((n, D))
    tC = np.zeros((D, K))
    R, tR = 0.0, 0.0
    if n_lab and kind in ("xent", "l2"):
        x = mu64[:, :K]
        if kind == "xent":
            terms = bce_with_logits(x, y)
            absterms = np.maximum(x, 0.0) + np.abs(x * y) + np.log1p(np.exp(-np.abs(x)))
            g, m = sigmoid(x) - y, sigmoid(x) + y
        else:
            terms = (x - y) ** 2
            absterms = terms
            g, m = 2.0 * (x - y), 2.0 * (np.abs(x) + y)
        R = s * terms[on].sum()
        tR = 8 * (n_lab * K) * U * s * absterms[on].sum()
        dmu[:, :K] = np.where(on[:, None], w * s * g, 0.0)
        mag[:, :K] = np.where(on[:, None], abs(w) * s * m, 0.0)
    elif n_lab and kind == "cov":
        mL, vL = mu64[on], v[on]
        cm, cv = mL - mL.mean(axis=0), vL - vL.mean(axis=0)
        C = cm.T @ cv / n_lab
        off = ~np.eye(D, K, dtype=bool)
        G = np.where(off, 2.0 * C, 0.0)
        R = (C[off] ** 2).sum()
        m2 = ((mL - mL[0]) ** 2).mean(axis=0)
        s2 = ((vL - vL[0]) ** 2).mean(axis=0)
        tC = 8 * n_lab * U * np.sqrt(m2[:, None] * s2[None, :])
        tR = (np.abs(G) * tC).sum() + 8 * D * K * U * abs(R)
        vc = np.zeros((n, K))
        vc[on] = cv
        dmu = (w / n_lab) * vc @ G.T
        mag = (abs(w) / n_lab) * np.abs(vc) @ np.abs(G).T
        prop = (abs(w) / n_lab) * np.abs(vc) @ np.where(off, 2.0 * tC, 0.0).T
    elif kind not in KINDS:
        raise ValueError(kind)
    return dict(R=R, n_lab=n_lab, C=C, G=G, dmu=dmu, mag=mag, prop=prop, tol_C=tC, tol_R=tR, on=on, K=K, D=D, n=n, y=y, v=v,
                sizes=sizes, scale=s, kind=kind, w=w)


def tol_dmu(ref, margin=1.0):
    """The module docstring's bound for the gradient of one regulariser() result, the fp32 part times `margin`."""
    return margin * GRAD_ULPS * V * ref["mag"] + ref["prop"] + TINY


def defined_zero(ref):
    """bool [n, D]: where dmu is an exact zero BY DEFINITION -- unlabelled rows and, for xent / l2, columns >= K."""
    z = np.repeat(~ref["on"][:, None], ref["D"], axis=1)
    if ref["kind"] != "cov":
        z[:, ref["K"]:] = True
    return z


def fp32_gradients(mu, ref):
    """The gradient stage of the device's formulas in numpy float32 -> dmu fp32 [n, D].  xent / l2: sigmoid, the label and the
    difference in fp32.  cov: G and the centred values are the fp64 ones rounded to fp32 ONCE (the covariance stage has a bound
    of its own, tol(C)); the products, their sum over k and the scale are fp32 operations."""
    f = np.float32
    n, D, K = ref["n"], ref["D"], ref["K"]
    out = np.zeros((n, D), f)
    if ref["n_lab"] == 0:
        return out
    ws = f(ref["w"]) * f(ref["scale"])
    on = ref["on"]
    if ref["kind"] == "cov":
        vc = np.zeros((n, K))
        vc[on] = ref["v"][on] - ref["v"][on].mean(axis=0)
        acc = np.zeros((n, D), f)
        G32, vc32 = ref["G"].astype(f), vc.astype(f)
        for k in range(K):
            acc = acc + vc32[:, k:k + 1] * G32[None, :, k]
        return (acc * (f(ref["w"]) / f(ref["n_lab"]))).astype(f)
    x = np.asarray(mu, f)[:, :K]
    y = ref["v"].astype(f) / ref["sizes"].astype(f)[None, :]
    with np.errstate(over="ignore"):
        g = (f(1) / (f(1) + np.exp(-x, dtype=f)) - y) if ref["kind"] == "xent" else f(2) * (x - y)
    out[:, :K] = np.where(on[:, None], ws * g, f(0))
    return out


def e32(kind, table_kind, n, D, lat_sizes, pattern, reduction="sum", w=1.0):
    """error / tol (margin 1) that fp32_gradients attains on one case."""
    mu = table(table_kind, n, D)
    rows = rows_for(n, lat_sizes, pattern)
    K = len(default_factors(lat_sizes))
    if K > D:
        return 0.0
    ref = regulariser(mu, rows, lat_sizes, kind, reduction, w)
    err = np.abs(fp32_gradients(mu, ref).astype(np.float64) - ref["dmu"])
    return float((err / (tol_dmu(ref) + 1e-300)).max())


# ---- torch, for autograd and the whole-step tests ----------------------------------------------------------------------------------
def regulariser_torch(mu, rows, lat_sizes, kind, reduction="sum", factors=None):
    """R (weight 1) as a differentiable torch scalar in mu's dtype; rows: numpy / list / tensor of row numbers."""
    import torch
    import torch.nn.functional as F
    rows = np.asarray(rows.cpu() if hasattr(rows, "cpu") else rows, np.int64)
    factors = default_factors(lat_sizes) if factors is None else list(factors)
    K = len(factors)
    on = labelled(rows)
    n_lab = int(on.sum())
    if n_lab == 0:
        return mu.sum() * 0
    idx = torch.tensor(np.nonzero(on)[0], device=mu.device)
    v = torch.tensor(values(rows[on], lat_sizes, factors), dtype=mu.dtype, device=mu.device)
    sizes = torch.tensor([int(lat_sizes[j]) for j in factors], dtype=mu.dtype, device=mu.device)
    mL = mu.index_select(0, idx)
    if kind == "xent":
        R = F.binary_cross_entropy_with_logits(mL[:, :K], v / sizes, reduction="sum")
    elif kind == "l2":
        R = ((mL[:, :K] - v / sizes) ** 2).sum()
    elif kind == "cov":
        C = (mL - mL.mean(dim=0, keepdim=True)).t() @ (v - v.mean(dim=0, keepdim=True)) / n_lab
        off = ~torch.eye(mu.shape[1], K, dtype=torch.bool, device=mu.device)
        return (C[off] ** 2).sum()
    else:
        raise ValueError(kind)
    return R / n_lab if reduction == "mean" else R


def semi_iteration_grads(hp, state, params, data, eps, rows):
    """oracle.disvae_oracle.train_iteration_grads for "s2vae": vae_forward + single_optimizer_loss("betaH", ...) with beta =
    hp["s2_beta"] + w_t R_sup -> (loss, logs, grads, outs); logs in the order SemiSupervisedVaeLoss stores them (recon_loss,
    kl_loss, kl_loss_i, sup_loss, n_labelled, loss).  rows None: all unlabelled."""
    from collections import OrderedDict

    import torch
    from oracle import disvae_oracle as O
    recon, (mu, logvar), z = O.vae_forward(params, data, eps)
    base, logs, _ = O.single_optimizer_loss("betaH", dict(hp, betaH_B=hp.get("s2_beta", 4)), state, data, recon, mu, logvar, z, True)
    gamma = float(hp.get("gamma_sup", 1.0))
    w = gamma
    if hp.get("sup_anneal", "fixed") == "anneal":
        w = O.linear_annealing(0, gamma, state.n_train_steps, hp.get("sup_anneal_steps", 0))
    if rows is None:
        R, n_lab = mu.sum() * 0, 0
    else:
        R = regulariser_torch(mu, rows, hp["lat_sizes"], hp.get("sup_loss", "xent"), hp.get("sup_reduction", "sum"), hp.get("sup_factors"))
        n_lab = int(labelled(np.asarray(rows)).sum())
    loss = base + w * R
    out_logs = OrderedDict((k, v.detach()) for k, v in logs.items() if k != "loss")
    out_logs["sup_loss"] = R.detach()
    out_logs["n_labelled"] = torch.tensor(float(n_lab), dtype=torch.float64)
    out_logs["loss"] = loss.detach()
    grads = torch.autograd.grad(loss, list(params.values()), allow_unused=True)
    grads = OrderedDict((k, g) for k, g in zip(params.keys(), grads))
    outs = dict(recon=recon.detach(), mu=mu.detach(), logvar=logvar.detach(), z=z.detach())
    return loss.detach(), out_logs, grads, outs
