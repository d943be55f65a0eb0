"""-m gpu: every kernel that takes (mu, logvar, z) at the inputs of a TRAINED model (tests/latent_regimes.py): active dimensions
with logvar -9 .. -12 and cluster means units apart beside collapsed ones in the same rows, plus hand-placed rows (tied maxima, an
outlier whose off-diagonal densities all underflow, logvar -20 / +4).  The rest of the suite runs these kernels at
initialisation-like inputs of magnitude 1.

Everything goes through the C-ABI at the smallest shapes that reach each kernel path and is held to the fp64 oracle at the
tolerance of the corresponding existing test, with two changes (latent_regimes.py): a per-dimension scale for [B, D] outputs, and
a measured margin -- the oracle is also evaluated in fp32 on the CPU (e32 = its worst error / tolerance) and the kernel passes at
ratio <= max(1, 4 e32); e32 > 2.5 fails the case as a wrong input.  Every element of every output is compared and must be finite."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from gpu_util import *  # noqa
from gpu_util import _lib  # noqa
from oracle import disvae_oracle as O
import latent_regimes as R
from test_gpu_fused_core import _fc_params, _fc_stage, _rand as _urand


def judge(what, got, ref64, ref32, rtol, atol_rel, per_dim=False):
    """got (device / cpu fp32) vs ref64 under the rule of latent_regimes.py; records like gpu_util.check."""
    got = got.detach().cpu()
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    assert torch.isfinite(got).all(), what + ": non-finite values"
    e32, _ = R.worst_ratio(ref32, ref64, rtol, atol_rel, per_dim)
    ratio, rel = R.worst_ratio(got, ref64, rtol, atol_rel, per_dim)
    record_stat("regime " + what, rel, ratio)
    print("regime %-34s e32 %8.3g  kernel %8.3g  bound %5.3g" % (what, e32, ratio, R.bound(e32)))
    assert math.isfinite(e32) and e32 <= R.CAP, "%s: wrong input: the fp32 oracle is %.3g x the tolerance from fp64" % (what, e32)
    assert ratio <= R.bound(e32), "%s: %.3g x the tolerance (bound %.3g, fp32 oracle %.3g), max err %.3g of the scale" % (
        what, ratio, R.bound(e32), e32, rel)


# ---- 1. beta-TCVAE estimator and gradient -------------------------------------------------------------------------------------
def _btcvae_run(z, mu, lv, n_data, mss, shards):
    """dvae_btcvae_fwd + _bwd over the row shards [(row0, rows)], every call with its own tmp -> [(rowstats, dz, dmu, dlv)]."""
    from disvae_amd.utils.math import log_importance_weights
    B, D = z.shape
    lw = torch.zeros(4); lw[:3] = log_importance_weights(B, n_data)
    c = R.BTCVAE_COEF
    coef = torch.zeros(_lib.NCOEF)
    coef[_lib.C_ALPHA], coef[_lib.C_BETA], coef[_lib.C_GAMMA], coef[_lib.C_ANNEAL] = c["alpha"], c["beta"], c["gamma"], c["anneal"]
    zd, mud, lvd, lwd, coefd = dev(z), dev(mu), dev(lv), dev(lw), dev(coef)
    rstride = _lib.rowstats_stride(D)
    out = []
    for row0, rows in shards:
        rs = torch.full((rows, rstride), float("nan"), device=DEV)
        tmp = torch.empty(_lib.btcvae_tmp_floats(B, rows, D), device=DEV)
        call("dvae_btcvae_fwd", ptr(zd), ptr(mud), ptr(lvd), B, D, row0, rows, int(mss), ptr(lwd), ptr(tmp), ptr(rs), stream())
        dz = torch.full((rows, D), float("nan"), device=DEV)
        dmu, dlv = torch.full((B, D), float("nan"), device=DEV), torch.full((B, D), float("nan"), device=DEV)
        call("dvae_btcvae_bwd", ptr(zd), ptr(mud), ptr(lvd), ptr(rs), B, D, row0, rows, int(mss), ptr(lwd), ptr(coefd), ptr(tmp),
             ptr(dz), ptr(dmu), ptr(dlv), stream())
        out.append((rs.cpu()[:, :4 + D], dz.cpu(), dmu.cpu(), dlv.cpu()))
    return out


def _btcvae_judge(tag, rs, dz, dmu, dlv, ref64, ref32):
    got = dict(zip(R.BTCVAE_FWD_NAMES, rs[:, :4].unbind(1)), lse_d=rs[:, 4:], dz=dz, dmu=dmu, dlv=dlv)
    for name in ref64:
        tol, per_dim = R.btcvae_tolerance(name)
        judge("%s %s" % (tag, name), got[name], ref64[name], ref32[name], per_dim=per_dim, **tol)


BTCVAE_CASES = [(B, D, n, kind, True) for (B, D, n) in R.BTCVAE_SHAPES for kind in R.KINDS] + [R.BTCVAE_SHAPES[0] + ("trained", False)]


@pytest.mark.parametrize("B,D,n_data,kind,mss", BTCVAE_CASES)
def test_btcvae_estimator_and_gradient(B, D, n_data, kind, mss):
    (z, mu, lv, _), ref64, ref32 = R.btcvae_case(kind, B, D, n_data, mss)
    (rs, dz, dmu, dlv), = _btcvae_run(z, mu, lv, n_data, mss, [(0, B)])
    _btcvae_judge("btcvae B=%d D=%d %s" % (B, D, kind) + ("" if mss else " no-mss"), rs, dz, dmu, dlv, ref64, ref32)


@pytest.mark.parametrize("kind", R.KINDS)
def test_btcvae_row_shards_at_513(kind):
    """Rows [0, 256) and [256, 513) of the B = 513 case (the data-parallel use; each shard takes the workgroup-per-row path the
    whole batch is too large for): forward rows bit-equal to the unsharded run, dz the concatenation, dmu / dlv the sum."""
    B, D, n_data = R.BTCVAE_SHAPES[2]
    assert B == 513
    (z, mu, lv, _), ref64, ref32 = R.btcvae_case(kind, B, D, n_data, True)
    (rs, _, _, _), = _btcvae_run(z, mu, lv, n_data, True, [(0, B)])
    (rsa, dza, dma, dla), (rsb, dzb, dmb, dlb) = _btcvae_run(z, mu, lv, n_data, True, [(0, 256), (256, B - 256)])
    assert torch.equal(rsa, rs[:256]) and torch.equal(rsb, rs[256:])
    _btcvae_judge("btcvae sharded B=513 %s" % kind, torch.cat((rsa, rsb)), torch.cat((dza, dzb)), dma + dmb, dla + dlb, ref64, ref32)


# ---- 2. reparameterisation and KL ---------------------------------------------------------------------------------------------
def _reparam_refs(mu, lv, eps, grads, g_dim, dtype):
    dz, dmx, dlx = (t.to(dtype) for t in grads)
    mr, lr = mu.to(dtype).requires_grad_(True), lv.to(dtype).requires_grad_(True)
    z = O.reparameterize(mr, lr, eps.to(dtype))
    kl_total, kl_dim = O.kl_normal_loss(mr, lr)
    ((z * dz).sum() + (mr * dmx).sum() + (lr * dlx).sum() + 2.5 * kl_total).backward(retain_graph=True)
    out = dict(z=z.detach(), kl_dim=kl_dim.detach(), kl_total=kl_total.detach().reshape(1), dmu=mr.grad.clone(), dlv=lr.grad.clone())
    mr.grad, lr.grad = None, None
    (kl_dim * g_dim.to(dtype)).sum().backward()
    out.update(kl_dmu=mr.grad, kl_dlv=lr.grad)
    return out


@pytest.mark.parametrize("kind", ["trained", "edges"])
@pytest.mark.parametrize("B,D", [(257, 10), (37, 17)])
def test_reparam_and_kl(B, D, kind):
    """dvae_reparam_kl_fwd (kl_dim and coef: two partial blocks at B = 257; the wide kernels at D = 17), the total through
    dvae_loss_epilogue, dvae_reparam_kl_bwd and dvae_kl_normal_bwd, at the tolerances of test_reparam_kl / test_reparam_kl_wide
    (the total: test_loss_epilogue_wide's rtol 1e-5)."""
    _, m_in, l_in, eps = R.family(kind, B, D, seed=2000 + B)
    ml = torch.stack((m_in, l_in), -1).reshape(B, 2 * D)
    grads = [torch.randn(B, D, generator=torch.Generator().manual_seed(s)) for s in (3, 4, 5)]
    g_dim = torch.randn(D, generator=torch.Generator().manual_seed(6))
    ref64 = _reparam_refs(m_in, l_in, eps, grads, g_dim, torch.float64)
    ref32 = _reparam_refs(m_in, l_in, eps, grads, g_dim, torch.float32)
    coef = torch.zeros(_lib.NCOEF); coef[_lib.C_INV_B] = 1.0 / B; coef[_lib.C_BETA] = 4.0; coef[_lib.C_ANNEAL] = 1.0
    mld, epsd, coefd = dev(ml), dev(eps), dev(coef)
    mu, lv, z = (torch.full((B, D), float("nan"), device=DEV) for _ in range(3))
    kl = torch.zeros(_lib.KL_FLOATS if D <= 16 else D, device=DEV)
    call("dvae_reparam_kl_fwd", ptr(mld), ptr(epsd), ptr(mu), ptr(lv), ptr(z), ptr(kl), ptr(coefd), B, D, stream())
    assert torch.equal(mu.cpu(), m_in) and torch.equal(lv.cpu(), l_in)
    tag = "reparam B=%d D=%d %s " % (B, D, kind)
    tol = dict(rtol=1e-4, atol_rel=2e-5)
    judge(tag + "z", z, ref64["z"], ref32["z"], per_dim=True, **tol)
    judge(tag + "kl_dim", kl[:D], ref64["kl_dim"], ref32["kl_dim"], **tol)
    packed, scal = torch.zeros(_lib.npack(D), device=DEV), torch.zeros(_lib.nscal(D), device=DEV)
    partials = torch.zeros(_lib.REC_NPART, device=DEV)
    call("dvae_loss_epilogue", _lib.LOSS_BETAH, ptr(partials), ptr(kl), 0, D, None, 0, None, B, ptr(coefd), ptr(packed), ptr(scal),
         stream())
    judge(tag + "kl_total", scal[_lib.S_KL:_lib.S_KL + 1], ref64["kl_total"], ref32["kl_total"], rtol=1e-5, atol_rel=0.0)
    sc = torch.zeros(_lib.NSCAL); sc[_lib.S_KLW] = 2.5
    dml = torch.full((B, 2 * D), float("nan"), device=DEV)
    call("dvae_reparam_kl_bwd", ptr(dev(grads[0])), None, None, ptr(dev(grads[1])), ptr(dev(grads[2])), ptr(dev(m_in)), ptr(dev(l_in)),
         ptr(epsd), ptr(dev(sc)), ptr(coefd), ptr(dml), B, D, stream())
    dm, dl = dml.cpu().view(B, D, 2).unbind(-1)
    judge(tag + "dmu", dm, ref64["dmu"], ref32["dmu"], per_dim=True, **tol)
    judge(tag + "dlv", dl, ref64["dlv"], ref32["dlv"], per_dim=True, **tol)
    kdm, kdl = torch.full((B, D), float("nan"), device=DEV), torch.full((B, D), float("nan"), device=DEV)
    call("dvae_kl_normal_bwd", ptr(dev(g_dim)), ptr(dev(m_in)), ptr(dev(l_in)), ptr(kdm), ptr(kdl), B, D, stream())
    judge(tag + "kl_normal_bwd dmu", kdm, ref64["kl_dmu"], ref32["kl_dmu"], per_dim=True, **tol)
    judge(tag + "kl_normal_bwd dlv", kdl, ref64["kl_dlv"], ref32["kl_dlv"], per_dim=True, **tol)


# ---- 3. the latent core inside the FC chain -----------------------------------------------------------------------------------
def _chain_refs(W, Bv, a, eps, acts, gd3, ext, mu_b, lv_b, n, D, dtype):
    """The restatement of test_fc_chain_forward / _backward in `dtype` (backward at the latent point (mu_b, lv_b))."""
    Wd = {k: v.to(dtype) for k, v in W.items()}
    Bd = {k: v.to(dtype) for k, v in Bv.items()}
    h1 = torch.relu(F.linear(a.to(dtype), Wd["e1"], Bd["e1"]))
    h2 = torch.relu(F.linear(h1, Wd["e2"], Bd["e2"]))
    ml = F.linear(h2, Wd["ml"], Bd["ml"])
    mu, lv = ml.view(n, D, 2).unbind(-1)
    z = mu + torch.exp(0.5 * lv) * eps.to(dtype)
    kl = (0.5 * (-1 - lv + mu * mu + torch.exp(lv))).sum(0)
    d1 = torch.relu(F.linear(z, Wd["d1"], Bd["d1"]))
    d2 = torch.relu(F.linear(d1, Wd["d2"], Bd["d2"]))
    d3 = torch.relu(F.linear(d2, Wd["d3"], Bd["d3"]))
    out = dict(h1=h1, h2=h2, ml=ml, mu=mu.contiguous(), logvar=lv.contiguous(), z=z, kl=kl, d1=d1, d2=d2, d3=d3)
    dz2, dmu_x, dlv_x = (t.to(dtype) for t in ext)
    gd2 = (gd3.to(dtype) @ Wd["d3"]) * (acts["d2"] > 0)
    gd1 = (gd2 @ Wd["d2"]) * (acts["d1"] > 0)
    dz = gd1 @ Wd["d1"]
    gz = dz + dz2
    klw = 1.7 / n
    m, l = mu_b.to(dtype), lv_b.to(dtype)
    dm = gz + klw * m + dmu_x
    dl = klw * 0.5 * (torch.exp(l) - 1) + gz * eps.to(dtype) * 0.5 * torch.exp(0.5 * l) + dlv_x
    dml = torch.stack((dm, dl), dim=-1).reshape(n, 2 * D)
    gh2 = (dml @ Wd["ml"]) * (acts["h2"] > 0)
    gh1 = (gh2 @ Wd["e2"]) * (acts["h1"] > 0)
    ga = (gh1 @ Wd["e1"]) * (acts["a_flat"] > 0)
    out.update(gd2=gd2, gd1=gd1, dz=dz, dml=dml, gh2=gh2, gh1=gh1, ga_flat=ga)
    return out


@pytest.mark.parametrize("n,D", [(20, 10), (1025, 10), (20, 6), (1025, 6)])
def test_fc_chain_latent_core(n, D):
    """dvae_fc_chain_fwd / _bwd (4 rows per workgroup at n = 20, 8 at n = 1025) with the regime made through the last encoder
    layer: bias -9 on the logvar entries of the active dimensions and 0 on the collapsed ones, the collapsed dimensions' weight
    rows (and their mu bias) scaled by 0.01.  The backward runs at the forward's own (mu, logvar) with the estimator's set of
    external latent gradients.  Tolerance of test_fc_chain_forward / _backward: rtol 1e-5, atol_rel 2e-6."""
    shapes, W, Bv = _fc_params(D, seed=3)
    A = R.n_active(D)
    Bv["ml"][1:2 * A:2] = -9.0
    W["ml"][2 * A:] *= 0.01
    Bv["ml"][2 * A::2] *= 0.01
    Bv["ml"][2 * A + 1::2] = 0.0
    ent = _fc_stage(shapes, W)
    a = torch.relu(_urand(n, 512, seed=1))
    eps = torch.randn(n, D, generator=torch.Generator().manual_seed(2))
    f = lambda *s: torch.full(s, float("nan"), device=DEV)
    out = dict(h1=f(n, 256), h2=f(n, 256), ml=f(n, 2 * D), mu=f(n, D), logvar=f(n, D), z=f(n, D), d1=f(n, 256), d2=f(n, 256), d3=f(n, 512))
    kl = torch.zeros(_lib.KL_FLOATS, device=DEV)
    bd = {k: dev(v) for k, v in Bv.items()}
    ad, ed = dev(a), dev(eps)
    st, addr = _lib.struct_of(_lib.FcChainFwdArgs, a_flat=ptr(ad), eps=ptr(ed), kl_part=ptr(kl) + 64, n_enc=n, n_kl=n, n_dec=n, D=D,
                              **{"w_" + k: ptr(ent[k][1]) for k in shapes}, **{"b_" + k: ptr(bd[k]) for k in shapes},
                              **{k: ptr(v) for k, v in out.items()})
    call("dvae_fc_chain_fwd", addr, stream())
    mu_b, lv_b = out["mu"].cpu(), out["logvar"].cpu()
    assert lv_b[:, :A].max().item() < -5.0 and lv_b[:, A:].abs().max().item() < 0.2 and mu_b[:, A:].abs().max().item() < 0.2
    # backward inputs (test_fc_chain_backward, extra = 1)
    gd3 = _urand(n, 512, seed=31)
    acts = {k: torch.relu(_urand(n, w, seed=10 + i)) for i, (k, w) in enumerate(
        [("d2", 256), ("d1", 256), ("h2", 256), ("h1", 256), ("a_flat", 512)])}
    ext = [_urand(n, D, seed=s) for s in (22, 24, 25)]                       # dz2, dmu_x, dlv_x
    ref64 = _chain_refs(W, Bv, a, eps, acts, gd3, ext, mu_b, lv_b, n, D, torch.float64)
    ref32 = _chain_refs(W, Bv, a, eps, acts, gd3, ext, mu_b, lv_b, n, D, torch.float32)
    tol = dict(rtol=1e-5, atol_rel=2e-6)
    tag = "chain n=%d D=%d " % (n, D)
    for k in ("h1", "h2", "d1", "d2", "d3"):
        judge(tag + k, out[k], ref64[k], ref32[k], **tol)
    for k in ("ml", "mu", "logvar", "z"):
        judge(tag + k, out[k], ref64[k], ref32[k], per_dim=True, **tol)
    rows = _lib.fc_chain_rows(n)
    assert rows == (4 if n <= 1024 else 8)
    nblk = (n + rows - 1) // rows
    parts = kl[16:16 + nblk * 16].view(nblk, 16).cpu().double()
    assert torch.all(parts[:, D:] == 0)
    judge(tag + "KL partial blocks", parts.sum(0)[:D], ref64["kl"], ref32["kl"], **tol)
    coef = torch.zeros(_lib.NCOEF); coef[_lib.C_INV_B] = 1.0 / n
    coefd = dev(coef)
    call("dvae_kl_finish", ptr(kl), nblk, ptr(coefd), D, stream())
    judge(tag + "KL finished", kl[:D], ref64["kl"] / n, ref32["kl"] / n, **tol)
    scal = torch.zeros(_lib.NSCAL); scal[_lib.S_KLW] = 1.7
    outb = dict(gd2=f(n, 256), gd1=f(n, 256), dz=f(n, D), dml=f(n, 2 * D), gh2=f(n, 256), gh1=f(n, 256), ga_flat=f(n, 512))
    ins = dict(gd3=dev(gd3), mu=dev(mu_b), logvar=dev(lv_b), eps=ed, dz2=dev(ext[0]), dz3=None, dmu_x=dev(ext[1]), dlv_x=dev(ext[2]),
               scal=dev(scal), coef=coefd, **{k: dev(v) for k, v in acts.items()})
    st2, addr2 = _lib.struct_of(_lib.FcChainBwdArgs, n=n, D=D, **{"w_" + k: ptr(ent[k][2]) for k in shapes},
                                **{k: ptr(v) for k, v in ins.items()}, **{k: ptr(v) for k, v in outb.items()})
    call("dvae_fc_chain_bwd", addr2, stream())
    for k in ("gd2", "gd1", "gh2", "gh1", "ga_flat"):
        judge(tag + "bwd " + k, outb[k], ref64[k], ref32[k], **tol)
    for k in ("dz", "dml"):
        judge(tag + "bwd " + k, outb[k], ref64[k], ref32[k], per_dim=True, **tol)


# ---- 4. marginal entropies ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["trained", "sharp"])
def test_latent_entropy(kind):
    """dvae_latent_entropy, N = 600, D = 5, S = 17 on samples drawn from the family, vs test_entropy_kernel_vs_oracle's
    restatement (O.estimate_latent_entropies) at its tolerance (rtol 1e-5, atol_rel 1e-6)."""
    N, D, S = 600, 5, 17
    z, mean, logvar, _ = R.family(kind, N, D, seed=4000)
    idx = torch.randperm(N, generator=torch.Generator().manual_seed(41))[:S]
    z_sd = z.index_select(0, idx).contiguous()
    ws = torch.empty(_lib.lib().dvae_latent_entropy_ws_floats(N, D, S), device=DEV)
    H = torch.full((D,), float("nan"), device=DEV)
    call("dvae_latent_entropy", ptr(dev(z_sd)), ptr(dev(mean)), ptr(dev(logvar)), N, D, S, ptr(ws), ptr(H), stream())
    ref64 = O.estimate_latent_entropies(z.double(), mean.double(), logvar.double(), idx, S, mini_batch_size=S)
    ref32 = O.estimate_latent_entropies(z, mean, logvar, idx, S, mini_batch_size=S)
    judge("entropy %s H" % kind, H, ref64, ref32, rtol=1e-5, atol_rel=1e-6)


# ---- 5. importance-weighted log-likelihood ------------------------------------------------------------------------------------
def test_iw_loglik():
    """dvae_iw_loglik, B = 10 images of (1, 32, 32), K = 37 samples, mu / logvar of the `trained` family (D = 10), on the
    per-row reconstruction terms dvae_recon_rows gives for random images; vs test_gpu_loglik.py's restatement of the fold
    (log w = -rec + log p(z) - log q(z|x), logsumexp - log K) at its tolerance: 2e-6 of the largest log w term of the image."""
    N, K, D, row = 10, 37, 10, 1 * 32 * 32
    _, mu, lv, _ = R.family("trained", N, D, seed=5000)
    g = torch.Generator().manual_seed(51)
    eps = torch.randn(N * K, D, generator=g)
    z = mu.repeat_interleave(K, 0) + torch.exp(0.5 * lv.repeat_interleave(K, 0)) * eps
    recon, target = dev(torch.rand(N * K, row, generator=g)), dev(torch.rand(N, row, generator=g))
    need = ctypes.c_long()
    call("dvae_recon_rows_ws_floats", N, K, row, ctypes.addressof(need))
    assert need.value == 0
    rec = torch.full((N * K,), float("nan"), device=DEV)
    call("dvae_recon_rows", ptr(recon), ptr(target), 0, N, K, row, _lib.REC["bernoulli"], None, ptr(rec), stream())
    state, ll = torch.full((N, 2), float("nan"), device=DEV), torch.full((N,), float("nan"), device=DEV)
    call("dvae_iw_loglik", ptr(dev(mu)), ptr(dev(lv)), ptr(dev(z)), ptr(dev(eps)), ptr(rec), N, K, D, K, 1, 1, ptr(state), ptr(ll), None,
         stream())
    rec32 = rec.cpu()
    assert torch.isfinite(rec32).all() and torch.isfinite(ll).all()

    def restated(dtype):
        r, zz, e, l = rec32.to(dtype).view(N, K), z.to(dtype), eps.to(dtype), lv.to(dtype)
        log_pz = (-0.5 * (zz ** 2).sum(1)).view(N, K)
        log_qz = (-0.5 * (e ** 2 + l.repeat_interleave(K, 0)).sum(1)).view(N, K)
        lw = -r + log_pz - log_qz
        return torch.logsumexp(lw, dim=1) - math.log(K), (r.abs() + log_pz.abs() + log_qz.abs()).max(dim=1).values

    want, scale = restated(torch.float64)
    want32, _ = restated(torch.float32)
    tol = 2e-6 * scale
    e32 = ((want32.double() - want).abs() / tol).max().item()
    ratio = ((ll.cpu().double() - want).abs() / tol).max().item()
    record_stat("regime iw_loglik", ((ll.cpu().double() - want).abs() / scale).max().item(), ratio)
    print("regime %-34s e32 %8.3g  kernel %8.3g  bound %5.3g" % ("iw_loglik", e32, ratio, R.bound(e32)))
    assert math.isfinite(e32) and e32 <= R.CAP, "wrong input: the fp32 restatement is %.3g x the tolerance from fp64" % e32
    assert ratio <= R.bound(e32), "worst error %.3g x tolerance (bound %.3g)" % (ratio, R.bound(e32))
