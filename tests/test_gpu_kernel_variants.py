"""-m gpu: parity on BOTH SIDES of every dispatch switch of the launchers (tests/kernel_variants.py lists the switches and, per
kernel instantiation, the test here or elsewhere that reaches it).  Every case is one or a few C-ABI calls on seeded inputs
against an fp64 torch-CPU reference of the same operation, outputs pre-filled with 7.0, at the last shape of one side of a
switch and the first of the other.  No tolerance is new: convs / linears / the FC chain rtol 1e-5 + 2e-6 max|ref| (K_RTOL /
K_ATOL of test_gpu_bench_sizes.py), the estimator the values of test_btcvae_fwd_bwd, Adam <= 1 ulp of torch's CPU Adam."""
import ctypes
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from gpu_util import *  # noqa
from gpu_util import _lib  # noqa
from oracle import disvae_oracle as O
from test_gpu_fused_core import _rand, _stage, _fc_params, _fc_stage
from test_gpu_mask_bits import _pack_bits

K_RTOL, K_ATOL = 1e-5, 2e-6       # = test_gpu_bench_sizes.py
KTOL = dict(rtol=K_RTOL, atol_rel=K_ATOL)


def full(*shape):
    return torch.full(shape, 7.0, device=DEV)


def _ws():
    return torch.empty(_lib.lib().dvae_conv_wgrad_ws_floats(), device=DEV)


# ---- estimator: launch_btcvae_bwd switches kernels at BTC_WG_MAX_ROWS = 512 local rows, DT = 10 / run-time D -----------------
N_DATA = 202599
BTC = dict(alpha=1.0, beta=6.4, gamma=1.5, anneal=0.37)


@functools.lru_cache(maxsize=None)
def _btc_problem(Bg, D, mss):
    """inputs and the fp64 row statistics / gradients of alpha*mi + beta*tc + anneal*gamma*dw over the WHOLE batch (computed
    once per (Bg, D, mss) and shared by the sharded and unsharded cases)."""
    g = torch.Generator().manual_seed(Bg)
    mu = torch.randn(Bg, D, generator=g)
    lv = torch.randn(Bg, D, generator=g) * 0.7 - 0.5
    eps = torch.randn(Bg, D, generator=g)
    z = mu + torch.exp(0.5 * lv) * eps
    dens = O.btcvae_log_densities(z.double(), mu.double(), lv.double(), N_DATA, mss)
    zr, mr, lr = (t.double().requires_grad_(True) for t in (z, mu, lv))
    mi, tc, dw = O.btcvae_terms(zr, mr, lr, N_DATA, mss)
    (BTC["alpha"] * mi + BTC["beta"] * tc + BTC["anneal"] * BTC["gamma"] * dw).backward()
    return z, mu, lv, [d.detach() for d in dens], zr.grad, mr.grad, lr.grad


def _btc_run(Bg, row0, Bl, D, mss):
    """dvae_btcvae_fwd then dvae_btcvae_bwd over the local rows [row0, row0 + Bl) -> (rowstats, dz, dmu, dlv)."""
    from disvae_amd.utils.math import log_importance_weights
    z, mu, lv = _btc_problem(Bg, D, mss)[:3]
    lw = torch.zeros(4); lw[:3] = log_importance_weights(Bg, N_DATA)
    coef = torch.zeros(_lib.NCOEF)
    coef[_lib.C_ALPHA], coef[_lib.C_BETA], coef[_lib.C_GAMMA], coef[_lib.C_ANNEAL] = BTC["alpha"], BTC["beta"], BTC["gamma"], BTC["anneal"]
    zd, mud, lvd, lwd, coefd = dev(z), dev(mu), dev(lv), dev(lw), dev(coef)
    rs, tmp = full(Bl, _lib.ROWSTATS), full(3 * D, Bg)
    call("dvae_btcvae_fwd", ptr(zd), ptr(mud), ptr(lvd), Bg, D, row0, Bl, int(mss), ptr(lwd), ptr(tmp), ptr(rs), stream())
    dz, dmu, dlv = full(Bl, D), full(Bg, D), full(Bg, D)
    call("dvae_btcvae_bwd", ptr(zd), ptr(mud), ptr(lvd), ptr(rs), Bg, D, row0, Bl, int(mss), ptr(lwd), ptr(coefd), ptr(tmp),
         ptr(dz), ptr(dmu), ptr(dlv), stream())
    torch.cuda.synchronize()
    return rs, dz, dmu, dlv


def _btc_check_rowstats(rs, dens, row0, Bl, tag):
    for k, nm in enumerate(["log_pz", "log_qz", "log_prod_qzi", "log_q_zCx"]):
        check(rs[:, k], dens[k][row0:row0 + Bl], rtol=2e-6, atol_rel=2e-6, what=tag + nm)


@pytest.mark.parametrize("Bg,D,mss", [(512, 10, True), (513, 10, True), (512, 6, True), (513, 6, True), (600, 16, True),
                                      (520, 1, True), (513, 6, False)])
def test_btcvae_bwd_at_the_row_switch(Bg, D, mss):
    """k_btcvae_bwd_wg<DT> up to 512 local rows, k_btcvae_bwd_rows<DT> + k_btcvae_bwd_cols<DT> above (loss.hip,
    launch_btcvae_bwd), DT = 10 for D = 10 and 0 (run-time D) otherwise."""
    _, _, _, dens, gz, gm, gl = _btc_problem(Bg, D, mss)
    rs, dz, dmu, dlv = _btc_run(Bg, 0, Bg, D, mss)
    tag = "btcvae Bg=%d D=%d mss=%d " % (Bg, D, mss)
    _btc_check_rowstats(rs, dens, 0, Bg, tag)
    check(dz, gz, rtol=2e-4, atol_rel=1e-5, what=tag + "dz")
    check(dmu, gm, rtol=2e-4, atol_rel=1e-5, what=tag + "dmu")
    check(dlv, gl, rtol=2e-4, atol_rel=1e-5, what=tag + "dlv")


@pytest.mark.parametrize("row0,Bl", [(0, 500), (500, 600)])
def test_btcvae_bwd_sharded_with_more_than_512_local_rows(row0, Bl):
    """Bg = 1100 rows, D = 6, as two row shards: [0, 500) on the workgroup-per-row kernel, [500, 1100) (600 local rows,
    Bl < Bg) on the wave-per-row pair.  Each case runs both shards (dz of the shards concatenated and dmu / dlv summed = the
    unsharded fp64 gradients) and checks its own shard's rows alone."""
    Bg, D = 1100, 6
    _, _, _, dens, gz, gm, gl = _btc_problem(Bg, D, True)
    rs, dz, dmu, dlv = _btc_run(Bg, row0, Bl, D, True)
    o0, ol = (500, 600) if row0 == 0 else (0, 500)
    rs_o, dz_o, dmu_o, dlv_o = _btc_run(Bg, o0, ol, D, True)
    _btc_check_rowstats(rs, dens, row0, Bl, "shard at row %d " % row0)
    check(dz, gz[row0:row0 + Bl], rtol=2e-4, atol_rel=1e-5, what="shard at row %d dz" % row0)      # its rows of dz are final
    check(torch.cat((dz, dz_o) if row0 == 0 else (dz_o, dz)), gz, rtol=2e-4, atol_rel=1e-5, what="sharded dz")
    check(dmu + dmu_o, gm, rtol=2e-4, atol_rel=1e-5, what="sharded dmu")
    check(dlv + dlv_o, gl, rtol=2e-4, atol_rel=1e-5, what="sharded dlv")


@pytest.mark.parametrize("B", [256, 257, 16384, 16385])
def test_reparam_kl_at_the_partial_block_switches(B):
    """reparam_kl_blocks (loss.hip): one workgroup per 256 rows (256 | 257: one | two partial blocks), capped at RK_BLOCKS = 64
    from 16384 rows (16385: the grid-stride loop takes a second trip)."""
    D = 10
    ml = _rand(B, 2 * D, seed=1, scale=1.5)
    eps = torch.randn(B, D, generator=torch.Generator().manual_seed(2))
    coef = torch.zeros(_lib.NCOEF); coef[_lib.C_INV_B] = 1.0 / B
    mu, lv, z = full(B, D), full(B, D), full(B, D)
    kl = full(16 + 64 * 16)
    call("dvae_reparam_kl_fwd", ptr(dev(ml)), ptr(dev(eps)), ptr(mu), ptr(lv), ptr(z), ptr(kl), ptr(dev(coef)), B, D, stream())
    m_ref, l_ref = ml.view(B, D, 2).unbind(-1)
    assert _lib.lib().dvae_reparam_kl_blocks(B) == min((B + 255) // 256, 64)
    assert torch.equal(mu.cpu(), m_ref) and torch.equal(lv.cpu(), l_ref)
    check(z, O.reparameterize(m_ref.double(), l_ref.double(), eps.double()), what="z B=%d" % B)
    check(kl[:D], O.kl_normal_loss(m_ref.double(), l_ref.double())[1], what="kl_dim B=%d" % B)


# ---- thin ends (C = 1 / 3 <-> 32 channels at 64x64): conv_thin_ws.hip takes over at N >= 192 -------------------------------
@functools.lru_cache(maxsize=1)
def _thin_problem(N, C):
    """seeded inputs of the thin-end bundle and its fp64 references (computed once per (N, C); the aligned and the misaligned
    run of one shape share them)."""
    x = torch.rand(N, C, 64, 64, generator=torch.Generator().manual_seed(1))
    w = _rand(32, C, 4, 4, seed=2, scale=0.2)
    b = _rand(32, seed=3, scale=0.1)
    dy = _rand(N, 32, 32, 32, seed=4)                         # NCHW values
    wr, br = w.double().requires_grad_(True), b.double().requires_grad_(True)
    pre = F.conv2d(x.double(), wr, br, stride=2, padding=1)
    ref = torch.relu(pre).detach()
    pre.backward(dy.double())
    a = torch.relu(_rand(N, 32, 32, 32, seed=5))              # NCHW values
    wt = _rand(32, C, 4, 4, seed=6, scale=0.2)
    g = _rand(N, C, 64, 64, seed=7)
    ar, wtr, btr = a.double().requires_grad_(True), wt.double().requires_grad_(True), torch.zeros(C, dtype=torch.float64, requires_grad=True)
    F.conv_transpose2d(ar, wtr, btr, stride=2, padding=1).backward(g.double())
    return dict(x=x, w=w, b=b, dy=dy, ref=ref, dw=wr.grad, db=br.grad, a=a, wt=wt, g=g, dx=(ar.grad * (a > 0)).detach(),
                dwt=wtr.grad, dbt=btr.grad)


def _off4(t=None, numel=None, dtype=torch.float32, fill=7.0):
    """(arena, view): the view starts 4 bytes into a 16-byte aligned arena (filled with `fill`) and holds `t` if given."""
    n = t.numel() if t is not None else numel
    arena = torch.full((n + 4,), fill, dtype=dtype, device=DEV)
    v = arena[1:1 + n]
    if t is not None:
        v.copy_(t.reshape(-1).to(DEV))
    assert ptr(arena) % 16 == 0 and ptr(v) % 16 == 4
    return keep(arena), v


def _thin_ends(N, C, misaligned=False):
    """conv1 forward (plain and with the bit plane), convT3's input gradient (fp32 mask, bit-plane mask) and both weight
    gradients with a thin side, each against fp64 at KTOL, outputs pre-filled with 7.0.  misaligned: the images (x, g), the
    outputs and the bit planes are views 4 bytes into their buffers, which launch_down_thin_ws / launch_wgrad_thin_ws decline
    (conv_thin_ws.hip: 16-byte LDS-DMA and stores), so k_down_thin<C, MODE> / k_wgrad_thin<C> run at any N.  Returns the
    forward outputs, the bit plane and the weight gradients."""
    P = _thin_problem(N, C)
    tag = "thin N=%d C=%d%s " % (N, C, " (4 bytes in)" if misaligned else "")
    ws = _ws()
    guards = []

    def inp(t):
        if not misaligned:
            return dev(t)
        return _off4(t)[1]

    def outp(*shape, dtype=torch.float32, fill=7.0):
        if not misaligned:
            return torch.full(shape, fill, dtype=dtype, device=DEV)
        arena, v = _off4(numel=math.prod(shape), dtype=dtype, fill=fill)
        guards.append((arena, fill))
        return v.view(*shape)

    # conv1: x[N,C,64,64] NCHW -> y[N,32,32,32] NHWC
    xd, wd, bd = inp(P["x"]), dev(P["w"]), dev(P["b"])
    y = outp(N, 32, 32, 32)
    call("dvae_conv4s2_fwd", ptr(xd), _lib.NCHW, ptr(wd), ptr(bd), ptr(y), _lib.NHWC, N, C, 64, 64, 32, _lib.ACT_RELU, stream())
    check(from_nhwc(y, N, 32, 32, 32), P["ref"], what=tag + "conv1 fwd", **KTOL)
    yb = outp(N, 32, 32, 32)
    bits = outp(N * 1024, dtype=torch.int32, fill=0x55555555)
    call("dvae_conv1_fwd_bits", ptr(xd), 0, ptr(wd), ptr(bd), ptr(yb), ptr(bits), N, C, stream())
    check(from_nhwc(yb, N, 32, 32, 32), P["ref"], what=tag + "conv1 fwd (bits)", **KTOL)
    assert torch.equal(bits, _pack_bits(yb))
    dw, db = full(32, C, 4, 4), full(32)
    call("dvae_conv4s2_wgrad", ptr(xd), _lib.NCHW, ptr(nhwc(P["dy"])), _lib.NHWC, ptr(dw), ptr(db), N, C, 64, 64, 32, ptr(ws), stream())
    check(dw, P["dw"], what=tag + "conv1 wgrad", **KTOL)
    check(db, P["db"], what=tag + "conv1 bias grad", **KTOL)
    # convT3: a[N,32,32,32] NHWC -> C x 64 x 64 NCHW; input gradient masked by a, weight gradient (bias from the big side)
    ad, gd, wtd = nhwc(P["a"]), inp(P["g"]), dev(P["wt"])
    dx = outp(N, 32, 32, 32)
    call("dvae_convT4s2_dgrad", ptr(gd), _lib.NCHW, ptr(wtd), ptr(ad), ptr(dx), _lib.NHWC, N, 32, 32, 32, C, stream())
    check(from_nhwc(dx, N, 32, 32, 32), P["dx"], what=tag + "convT3 dgrad", **KTOL)
    dxb = outp(N, 32, 32, 32)
    mbits = _pack_bits(ad)
    if misaligned:
        mbits = _off4(mbits, dtype=torch.int32, fill=0)[1]
    call("dvae_convT3_dgrad_bits", ptr(gd), ptr(wtd), ptr(mbits), ptr(dxb), N, C, stream())
    check(from_nhwc(dxb, N, 32, 32, 32), P["dx"], what=tag + "convT3 dgrad (bits)", **KTOL)
    dwt, dbt = full(32, C, 4, 4), full(C)
    call("dvae_convT4s2_wgrad", ptr(ad), _lib.NHWC, ptr(gd), _lib.NCHW, ptr(dwt), ptr(dbt), N, 32, 32, 32, C, ptr(ws), stream())
    check(dwt, P["dwt"], what=tag + "convT3 wgrad", **KTOL)
    check(dbt, P["dbt"], what=tag + "convT3 bias grad", **KTOL)
    for arena, fill in guards:
        assert arena[0].item() == fill and torch.all(arena[-3:] == fill), tag + "the elements around a 4-byte-in output are untouched"
    return dict(y=y, yb=yb, bits=bits, dx=dx, dxb=dxb, dw=dw, dwt=dwt)


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("N", [191, 192])
def test_thin_ends_at_the_wave_specialised_switch(N, C):
    """conv1 forward (plain and with the bit plane), convT3's input gradient (fp32 mask, bit-plane mask) and both weight
    gradients with a thin side: k_down_thin<C, MODE> / k_wgrad_thin<C> at 191 images, k_down_thin_ws<C, MODE> /
    k_wgrad_thin_ws<C, BIAS_BIG> at 192 (launch_down_thin_ws / launch_wgrad_thin_ws: N >= 192; a fp32 mask stays on
    k_down_thin<C, 1> on both sides)."""
    _thin_ends(N, C)


@pytest.mark.parametrize("N,C", [(193, 1), (193, 3), (224, 3), (256, 1), (257, 1), (257, 3), (320, 3)])
def test_thin_ends_past_the_wave_specialised_switch(N, C):
    """The same bundle at the trip counts of the two wave-specialised kernels that 192 images (3 / 6 trips in every workgroup)
    leave out.  k_down_thin_ws: 512 workgroups, image lane n0 = (b & 7) + 8 (b >> 6) in 0..63, ceil((N - n0) / 64) trips
    through a ring of four tile stages and two output stages picked by the parity of the trip; k_wgrad_thin_ws: 256 workgroups,
    n0 in 0..31, ceil((N - n0) / 32) trips through a ring of three.
      N = 193: 4 | 3 and 7 | 6 trips (workgroups of image lane 0 against the rest);  224: 4 | 3 and 7 everywhere;
      256: 4 everywhere (the ring depth) and 8;  257: 5 | 4 and 9 | 8;  320: 5 everywhere (odd, above the ring depth) and 10.
    The fp32-mask input gradient stays on k_down_thin<C, 1>: min(8 N, 1536) workgroups, so 193 images are also its first
    case past the cap (workgroups 0..7 take a second unit), as they are of k_wgrad_thin_reduce behind a full partial buffer."""
    _thin_ends(N, C)


def test_thin_ends_past_the_cap_on_buffers_the_wave_specialised_kernels_decline():
    """N = 193, C = 3 with the images, the outputs and the bit planes 4 bytes into their buffers: modes 0, 2 and 3 of the fp32
    k_down_thin and k_wgrad_thin<3, float>, which aligned buffers reach only below 192 images, past their grid caps (1544
    units on 1536 workgroups; 1544 on WT_MAX_BLOCKS = 512: 4 | 3 trips).  conv_thin_ws.hip's header states that
    k_down_thin_ws accumulates in k_down_thin's order and gives the same bits: the forward outputs, the emitted bit plane and
    the bit-masked input gradient of the two runs are compared with torch.equal.  The weight gradients are not: k_wgrad_thin_ws
    sums 16x16x4 tiles, k_wgrad_thin 32x32x2 tiles, in another order (its header promises k_wgrad_thin's partial-buffer LAYOUT
    only), so they are held to fp64 alone."""
    al = _thin_ends(193, 3)
    mis = _thin_ends(193, 3, misaligned=True)
    for k in ("y", "yb", "bits", "dxb"):
        assert torch.equal(al[k], mis[k]), "k_down_thin_ws and k_down_thin differ in " + k
    assert torch.equal(al["dx"], mis["dx"])                 # k_down_thin<3, 1> both times: alignment changes nothing


# ---- 32-channel weight gradients: grid cap of conv_wgrad_ws.hip, reduction form of wgrad_reduce.h ---------------------------
def _wgrad32(N, Hs, transposed, small_nchw=False):
    """conv (transposed = False: x big, dy small, bias from the small side) or convT (x small, dy big, bias from the big side)
    weight gradient between Hb = 2 Hs and Hs, 32 <-> 32 channels, against autograd in fp64."""
    Hb = 2 * Hs
    big, small = _rand(N, 32, Hb, Hb, seed=1), _rand(N, 32, Hs, Hs, seed=2)
    w = torch.zeros(32, 32, 4, 4, dtype=torch.float64, requires_grad=True)
    bias = torch.zeros(32, dtype=torch.float64, requires_grad=True)
    if transposed:
        F.conv_transpose2d(small.double(), w, bias, stride=2, padding=1).backward(big.double())
    else:
        F.conv2d(big.double(), w, bias, stride=2, padding=1).backward(small.double())
    sd, sl = (dev(small), _lib.NCHW) if small_nchw else (nhwc(small), _lib.NHWC)
    dw, db = full(32, 32, 4, 4), full(32)
    if transposed:
        call("dvae_convT4s2_wgrad", ptr(sd), sl, ptr(nhwc(big)), _lib.NHWC, ptr(dw), ptr(db), N, 32, Hs, Hs, 32, ptr(_ws()), stream())
    else:
        call("dvae_conv4s2_wgrad", ptr(nhwc(big)), _lib.NHWC, ptr(sd), sl, ptr(dw), ptr(db), N, 32, Hb, Hb, 32, ptr(_ws()), stream())
    tag = "%s wgrad N=%d HS=%d%s " % ("convT" if transposed else "conv", N, Hs, " NCHW small" if small_nchw else "")
    check(dw, w.grad, what=tag + "dw", **KTOL)
    check(db, bias.grad, what=tag + "db", **KTOL)


@pytest.mark.parametrize("Hs", [16, 8])
@pytest.mark.parametrize("N", [128, 129, 320, 321])
def test_conv_wgrad32_at_the_grid_cap(N, Hs):
    """k_wgrad32ws<HS>: min(units, 256) workgroups, min(units, 192) for 128 < N <= 320 (conv_wgrad_ws.hip, launch_wgrad_ws_t)."""
    _wgrad32(N, Hs, transposed=False)


@pytest.mark.parametrize("Hs", [16, 8])
@pytest.mark.parametrize("N", [129, 321])
def test_convT_wgrad32_at_the_grid_cap(N, Hs):
    _wgrad32(N, Hs, transposed=True)


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("Hs,small_nchw", [(8, False), (4, False), (4, True)])
@pytest.mark.parametrize("N", [767, 768])
def test_wgrad32_at_the_reduction_form_switch(N, Hs, small_nchw, transposed):
    """k_wgrad32_reduce<false> below WGR_LEAN_MIN_IMAGES = 768 images, k_wgrad32_reduce<true> from there (launch_wgrad32_reduce),
    behind k_wgrad32ws<8> and behind k_wgrad32<4> (conv_mfma.hip) with the 4x4 side NHWC and NCHW."""
    _wgrad32(N, Hs, transposed, small_nchw)


# ---- FC chain: 4 rows per workgroup up to 1024 rows, 8 above (fc_chain_rows) --------------------------------------------------
@pytest.mark.parametrize("ends", [False, True])
@pytest.mark.parametrize("n,D", [(1024, 10), (1025, 10), (1024, 6), (1025, 6)])
def test_fc_chain_at_the_row_group_switch(n, D, ends):
    """k_fc_chain_fwd / _bwd<8, 2, RG, CONV>: RG = 1 up to FCC_R4_MAX_ROWS = 1024 rows, RG = 2 above; CONV = the 4x4 ends of the
    conv stacks in the same launch.  Forward and backward against fp64 (with the ends: through the 8x8 <-> 4x4 layers)."""
    assert _lib.fc_chain_rows(n) == (4 if n <= 1024 else 8)
    shapes, W, Bv = _fc_params(D, seed=3)
    ent = _fc_stage(shapes, W)
    bd = {k: dev(v) for k, v in Bv.items()}
    Wd = {k: v.double() for k, v in W.items()}
    Bd = {k: v.double() for k, v in Bv.items()}
    tag = "chain n=%d D=%d ends=%d " % (n, D, ends)
    eps = torch.randn(n, D, generator=torch.Generator().manual_seed(2))
    epsd = dev(eps)
    if ends:
        wc, wt = _rand(32, 32, 4, 4, seed=31, scale=0.2), _rand(32, 32, 4, 4, seed=32, scale=0.2)
        bc, bt = _rand(32, seed=33, scale=0.1), _rand(32, seed=34, scale=0.1)
        wcd, wtd, bcd, btd = dev(wc), dev(wt), dev(bc), dev(bt)
        img = {k: torch.empty(16384, device=DEV) for k in ("c_down", "c_up", "t_down", "t_up")}
        _stage([(wcd, img["c_down"], img["c_up"]), (wtd, img["t_down"], img["t_up"])])
        conv_in = torch.relu(_rand(n, 32, 8, 8, seed=41))                       # NCHW values
        a = torch.relu(F.conv2d(conv_in.double(), wc.double(), bc.double(), stride=2, padding=1)).reshape(n, 512)
    else:
        a = torch.relu(_rand(n, 512, seed=1)).double()
    # ---- forward
    out = dict(h1=full(n, 256), h2=full(n, 256), ml=full(n, 2 * D), mu=full(n, D), logvar=full(n, D), z=full(n, D),
               d1=full(n, 256), d2=full(n, 256), d3=full(n, 512))
    kl = full(_lib.KL_FLOATS)
    a_flat = full(n, 512) if ends else dev(a.float())
    up = full(n, 8, 8, 32)
    extra = {}
    if ends:
        extra = dict(conv_in=ptr(nhwc(conv_in)), conv_w=ptr(img["c_down"]), conv_b=ptr(bcd), convT_w=ptr(img["t_up"]), convT_b=ptr(btd),
                     convT_out=ptr(up))
    st, addr = _lib.struct_of(_lib.FcChainFwdArgs, a_flat=ptr(a_flat), eps=ptr(epsd), kl_part=ptr(kl) + 64, n_enc=n, n_kl=n, n_dec=n, D=D,
                              **{"w_" + k: ptr(ent[k][1]) for k in shapes}, **{"b_" + k: ptr(bd[k]) for k in shapes},
                              **{k: ptr(v) for k, v in out.items()}, **extra)
    call("dvae_fc_chain_fwd", addr, stream())
    if ends:
        check(a_flat, a, what=tag + "a_flat", **KTOL)             # the 8x8 -> 4x4 layer against fp64 ...
    a = a_flat.cpu().double()                                     # ... and the FC stack on the fp32 values it read
    h1 = torch.relu(F.linear(a, Wd["e1"], Bd["e1"]))
    h2 = torch.relu(F.linear(h1, Wd["e2"], Bd["e2"]))
    ml = F.linear(h2, Wd["ml"], Bd["ml"])
    mu, lv = ml.view(n, D, 2).unbind(-1)
    z = mu + torch.exp(0.5 * lv) * eps.double()
    d1 = torch.relu(F.linear(z, Wd["d1"], Bd["d1"]))
    d2 = torch.relu(F.linear(d1, Wd["d2"], Bd["d2"]))
    d3 = torch.relu(F.linear(d2, Wd["d3"], Bd["d3"]))
    if ends:
        ref_up = torch.relu(F.conv_transpose2d(d3.view(n, 32, 4, 4), wt.double(), bt.double(), stride=2, padding=1))
        check(from_nhwc(up, n, 32, 8, 8), ref_up, what=tag + "convT out", **KTOL)
    for k, ref in (("h1", h1), ("h2", h2), ("ml", ml), ("mu", mu), ("logvar", lv), ("z", z), ("d1", d1), ("d2", d2), ("d3", d3)):
        check(out[k], ref, what=tag + k, **KTOL)
    rows = _lib.fc_chain_rows(n)
    nblk = (n + rows - 1) // rows
    parts = kl[16:16 + nblk * 16].view(nblk, 16).cpu().double()
    check(parts.sum(0)[:D], (0.5 * (-1 - lv + mu * mu + torch.exp(lv))).sum(0), what=tag + "KL partial blocks", **KTOL)
    assert torch.all(parts[:, D:] == 0)
    # ---- backward
    acts = {k: torch.relu(_rand(n, wd_, seed=60 + i)) for i, (k, wd_) in enumerate(
        [("d2", 256), ("d1", 256), ("h2", 256), ("h1", 256), ("a_flat", 512), ("d3", 512)])}
    bmu, blv, dz2 = _rand(n, D, seed=20), _rand(n, D, seed=21, scale=0.7), _rand(n, D, seed=22)
    scal = torch.zeros(_lib.NSCAL); scal[_lib.S_KLW] = 1.7
    coef = torch.zeros(_lib.NCOEF); coef[_lib.C_INV_B] = 1.0 / n
    bout = dict(gd2=full(n, 256), gd1=full(n, 256), dz=full(n, D), dml=full(n, 2 * D), gh2=full(n, 256), gh1=full(n, 256),
                ga_flat=full(n, 512))
    gin = full(n, 8, 8, 32)
    extra = {}
    if ends:
        gout = _rand(n, 32, 8, 8, seed=51)                                       # NCHW values
        conv_act = torch.relu(_rand(n, 32, 8, 8, seed=71))
        gd3 = F.conv2d(gout.double(), wt.double(), None, stride=2, padding=1).reshape(n, 512) * (acts["d3"] > 0)
        gd3d = full(n, 512)
        extra = dict(convT_gout=ptr(nhwc(gout)), convT_w=ptr(img["t_down"]), d3=ptr(dev(acts["d3"])), conv_w=ptr(img["c_up"]),
                     conv_act=ptr(nhwc(conv_act)), conv_gin=ptr(gin))
    else:
        gd3 = _rand(n, 512, seed=1).double()
        gd3d = dev(gd3.float())
    ins = dict(gd3=gd3d, mu=dev(bmu), logvar=dev(blv), eps=epsd, dz2=dev(dz2), scal=dev(scal), coef=dev(coef),
               **{k: dev(v) for k, v in acts.items() if k != "d3"})
    st2, addr2 = _lib.struct_of(_lib.FcChainBwdArgs, n=n, D=D, **{"w_" + k: ptr(ent[k][2]) for k in shapes},
                                **{k: ptr(v) for k, v in ins.items()}, **{k: ptr(v) for k, v in bout.items()}, **extra)
    call("dvae_fc_chain_bwd", addr2, stream())
    gd2 = (gd3 @ Wd["d3"]) * (acts["d2"] > 0)
    gd1 = (gd2 @ Wd["d2"]) * (acts["d1"] > 0)
    dz = gd1 @ Wd["d1"]
    gz = dz + dz2.double()
    klw = 1.7 / n
    m, l = bmu.double(), blv.double()
    dm = gz + klw * m
    dl = klw * 0.5 * (torch.exp(l) - 1) + gz * eps.double() * 0.5 * torch.exp(0.5 * l)
    dml = torch.stack((dm, dl), dim=-1).reshape(n, 2 * D)
    gh2 = (dml @ Wd["ml"]) * (acts["h2"] > 0)
    gh1 = (gh2 @ Wd["e2"]) * (acts["h1"] > 0)
    ga = (gh1 @ Wd["e1"]) * (acts["a_flat"] > 0)
    if ends:
        check(gd3d, gd3, what=tag + "bwd gd3", **KTOL)
        ref_gin = F.conv_transpose2d(ga.view(n, 32, 4, 4), wc.double(), None, stride=2, padding=1) * (conv_act > 0)
        check(from_nhwc(gin, n, 32, 8, 8), ref_gin, what=tag + "bwd conv_gin", **KTOL)
    for k, ref in (("gd2", gd2), ("gd1", gd1), ("dz", dz), ("dml", dml), ("gh2", gh2), ("gh1", gh1), ("ga_flat", ga)):
        check(bout[k], ref, what=tag + "bwd " + k, **KTOL)


# ---- linears ------------------------------------------------------------------------------------------------------------------
def _linear(M, K, N, act=_lib.ACT_RELU, parts=("fwd", "dgrad", "wgrad")):
    """dvae_linear_fwd / _dgrad / _wgrad, each without and with the workspace, against fp64."""
    tag = "linear M=%d K=%d N=%d " % (M, K, N)
    x = _rand(M, K, seed=1)
    w = _rand(N, K, seed=2, scale=1 / math.sqrt(K))
    b = _rand(N, seed=3, scale=0.1)
    dy = _rand(M, N, seed=4)
    xact = _rand(M, K, seed=5)
    xd, wd, bd, dyd, xactd = dev(x), dev(w), dev(b), dev(dy), dev(xact)
    ws = _ws()
    x64, w64, dy64 = x.double(), w.double(), dy.double()
    if "fwd" in parts:
        pre = F.linear(x64, w64, b.double())
        ref = {_lib.ACT_NONE: pre, _lib.ACT_RELU: torch.relu(pre), _lib.ACT_LEAKY02: F.leaky_relu(pre, 0.2)}[act]
        for wsp in (None, ptr(ws)):
            y = full(M, N)
            call("dvae_linear_fwd", ptr(xd), ptr(wd), ptr(bd), ptr(y), M, K, N, act, wsp, stream())
            check(y, ref, what=tag + "fwd ws=%d" % (wsp is not None), **KTOL)
    if "wgrad" in parts:
        rw, rb = dy64.t() @ x64, dy64.sum(0)
        for wsp in (None, ptr(ws)):
            dw, db = full(N, K), full(N)
            call("dvae_linear_wgrad", ptr(xd), ptr(dyd), ptr(dw), ptr(db), M, K, N, wsp, stream())
            check(dw, rw, what=tag + "wgrad ws=%d" % (wsp is not None), **KTOL)
            check(db, rb, what=tag + "bias grad ws=%d" % (wsp is not None), **KTOL)
    if "dgrad" in parts:
        rx = dy64 @ w64
        for mact in (_lib.ACT_NONE, _lib.ACT_RELU, _lib.ACT_LEAKY02):
            mult = {0: torch.ones_like(xact), 1: (xact > 0).float(), 2: torch.where(xact > 0, 1.0, 0.2)}[mact].double()
            for wsp in (None, ptr(ws)):
                dx = full(M, K)
                call("dvae_linear_dgrad", ptr(dyd), ptr(wd), ptr(xactd) if mact else None, mact, ptr(dx), M, K, N, wsp, stream())
                check(dx, rx * mult, what=tag + "dgrad act=%d ws=%d" % (mact, wsp is not None), **KTOL)


@pytest.mark.parametrize("Kc", [32, 36, 64, 68, 128, 132, 256, 260, 512, 516])
def test_linear_at_the_contraction_length_switches(Kc):
    """try_fc32 (linear.hip): k_fc32<KP> with KP = 32 / 64 / 128 / 256 / 512 = the contraction length rounded up, nothing above
    512.  K = N = Kc: the forward contracts over K, the input gradient over N (into an aligned output: SC = 0)."""
    _linear(40, Kc, Kc, parts=("fwd", "dgrad"))


@pytest.mark.parametrize("Kc", [32, 64, 128, 256, 512])
def test_linear_dgrad_into_a_narrow_unaligned_output(Kc):
    """k_fc32<KP, true, 2>: the input gradient over N = Kc into K = 10 columns (the decoder's first layer), and the forward
    of that layer (k_fc32<32, false, 1>: a short unaligned contraction)."""
    _linear(40, 10, Kc, parts=("fwd", "dgrad"))


@pytest.mark.parametrize("M", [64, 65, 4096, 4100])
def test_linear_wgrad_at_the_batch_switches(M):
    """try_fcw32: k_fcw32<64> up to 64 rows, k_fcw32<256> up to 4096, above the split-contraction k_gemm<false, true>."""
    _linear(M, 256, 48, parts=("wgrad",))


@pytest.mark.parametrize("M,K,N,parts", [(2048, 64, 960, ("fwd",)), (2048, 64, 1024, ("fwd",)),
                                         (2048, 960, 64, ("dgrad",)), (2048, 1024, 64, ("dgrad",)),
                                         (40, 2048, 960, ("wgrad",)), (40, 2048, 1024, ("wgrad",))])
def test_linear_at_the_output_tile_count_switch(M, K, N, parts):
    """try_fc32 / try_fcw32 leave outputs of >= 512 64x64 tiles (32 x 15 = 480 | 32 x 16 = 512) to the 64x64-tile k_gemm."""
    _linear(M, K, N, parts=parts)


@pytest.mark.parametrize("M", [63, 64, 704, 705, 1664, 1665])
def test_discriminator_linear_at_the_tile_switches(M):
    """gemm_dma.hip at N = K = 1000: k_gdma tiles of 32 / 64 / 128 rows from ceil(M / tile) * 16 (704 | 705, 1664 | 1665);
    k_gdma_wg takes the weight gradient from 64 rows (63: k_fcw32<64>)."""
    _linear(M, 1000, 1000, act=_lib.ACT_LEAKY02)


@pytest.mark.parametrize("K", [252, 256])
def test_narrow_output_linear_at_its_minimum_contraction(K):
    """linear_narrow.hip (N = 2 outputs, the discriminator's last layer) from K = 256; below, k_fc32."""
    _linear(100, K, 2, act=_lib.ACT_NONE)


@pytest.mark.parametrize("M,K,N", [(40, 1000, 36), (40, 301, 36), (100, 256, 8), (100, 256, 9)])
def test_linear_outside_the_lds_resident_kernels(M, K, N):
    """What is left after try_narrow / try_fc32 / try_gdma: a long aligned contraction into few columns (k_gemm32<true, true>
    forward, k_gemm<true, true> + k_splitk_epilogue input gradient), a contraction that is no multiple of 4 (k_gemm<true,
    false> + k_splitk_epilogue), and the narrow kernels' widest output (NARROW_MAX = 8 | 9 columns)."""
    _linear(M, K, N, act=_lib.ACT_LEAKY02)


@pytest.mark.parametrize("N,Hs", [(64, 16), (65, 16), (256, 8), (257, 8), (1024, 4), (1025, 4),
                                  (128, 16), (129, 16), (192, 16), (193, 16), (256, 16), (320, 16), (513, 8), (2049, 4)])
def test_conv32_at_the_persistent_grid_switch(N, Hs):
    """The 32 <-> 32 channel forward / input-gradient kernels run min(units, 256) persistent workgroups (launch_down_dma_t,
    launch_up_ws_t, launch_down_t<4>, launch_up_t<4>): one unit per workgroup up to N * Hs * Hs / 64 = 256, the first
    workgroup takes a second unit at the next image count.
    Further trip counts of the software-pipelined loops (k_down32dma: a ring of three tile buffers; k_up32ws: two input and
    two output stages, the tile after next in registers), HS 16 = 4 N units: 128 / 192 / 256 / 320 images are 2 / 3 / 4 / 5
    trips in every workgroup, 129 and 193 are 3 | 2 and 4 | 3 (workgroups 0..3 against the rest); HS 8: 513 images are 3 | 2;
    HS 4: 2049 images = 513 units are 3 | 2.  None of these was held to fp64 before: test_gpu_bench_sizes.py runs 261 and 1024
    images at HS 16 (5 | 4, 16), 1027 / 1100 at HS 8 (5 | 4), 4099 / 4200 at HS 4 (5 | 4), and
    test_conv32_on_staged_images_is_bit_identical_to_the_raw_weight_path compares two runs of one kernel."""
    Hb = 2 * Hs
    tag = "conv32 N=%d HS=%d " % (N, Hs)
    w, b = _rand(32, 32, 4, 4, seed=2, scale=0.2), _rand(32, seed=3, scale=0.1)
    wd, bd = dev(w), dev(b)
    big, small = _rand(N, 32, Hb, Hb, seed=1), torch.relu(_rand(N, 32, Hs, Hs, seed=5))
    bigd, smalld = nhwc(big), nhwc(small)
    # down: Conv2d forward (bias + ReLU), ConvTranspose2d input gradient (masked by the small-side activation)
    y = full(N, Hs, Hs, 32)
    call("dvae_conv4s2_fwd", ptr(bigd), _lib.NHWC, ptr(wd), ptr(bd), ptr(y), _lib.NHWC, N, 32, Hb, Hb, 32, _lib.ACT_RELU, stream())
    down = F.conv2d(big.double(), w.double(), None, stride=2, padding=1)
    check(from_nhwc(y, N, 32, Hs, Hs), torch.relu(down + b.double().view(1, 32, 1, 1)), what=tag + "conv fwd", **KTOL)
    dx = full(N, Hs, Hs, 32)
    call("dvae_convT4s2_dgrad", ptr(bigd), _lib.NHWC, ptr(wd), ptr(smalld), ptr(dx), _lib.NHWC, N, 32, Hs, Hs, 32, stream())
    check(from_nhwc(dx, N, 32, Hs, Hs), down * (small > 0), what=tag + "convT dgrad", **KTOL)
    # up: ConvTranspose2d forward, Conv2d input gradient (masked by the big-side activation)
    yu = full(N, Hb, Hb, 32)
    call("dvae_convT4s2_fwd", ptr(smalld), _lib.NHWC, ptr(wd), ptr(bd), ptr(yu), _lib.NHWC, N, 32, Hs, Hs, 32, _lib.ACT_RELU, stream())
    up = F.conv_transpose2d(small.double(), w.double(), None, stride=2, padding=1)
    check(from_nhwc(yu, N, 32, Hb, Hb), torch.relu(up + b.double().view(1, 32, 1, 1)), what=tag + "convT fwd", **KTOL)
    du = full(N, Hb, Hb, 32)
    call("dvae_conv4s2_dgrad", ptr(smalld), _lib.NHWC, ptr(wd), ptr(bigd), ptr(du), _lib.NHWC, N, 32, Hb, Hb, 32, stream())
    check(from_nhwc(du, N, 32, Hb, Hb), up * (big > 0), what=tag + "conv dgrad", **KTOL)


@pytest.mark.parametrize("N", [7, 8, 256, 260])
def test_generic_wgrad_at_the_chunk_switches(N):
    """launch_wgrad_generic (32x32 single-channel images, the MNIST geometry): N * 16 * 16 / 1024 position chunks --
    k_wgrad_generic + k_chansum below two chunks (7 images), k_wgrad_generic_part / _fin from 8, at most 64 chunks (256 | 260)."""
    x = torch.rand(N, 1, 32, 32, generator=torch.Generator().manual_seed(1))
    dy = _rand(N, 32, 16, 16, seed=4)
    w = torch.zeros(32, 1, 4, 4, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(32, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), w, b, stride=2, padding=1).backward(dy.double())
    dw, db = full(32, 1, 4, 4), full(32)
    call("dvae_conv4s2_wgrad", ptr(dev(x)), _lib.NCHW, ptr(nhwc(dy)), _lib.NHWC, ptr(dw), ptr(db), N, 1, 32, 32, 32, ptr(_ws()), stream())
    # (rtol 1e-4 + 2e-5 max|ref|: the tolerance test_conv_fwd_dgrad_wgrad holds these shape-generic kernels to)
    check(dw, w.grad, what="generic wgrad N=%d dw" % N)
    check(db, b.grad, what="generic wgrad N=%d db" % N)


@pytest.mark.parametrize("M", [65, 129])
def test_linear_wgrad_grouped_past_its_slab_switches(M):
    """launch_linear_wgrad_grouped: k_fcw_grouped<64> up to 64 rows, <128> up to 128, <256> above (test_linear_wgrad_grouped
    runs 64 and 128; here the first row count of the next variant)."""
    shapes = [(512, 256), (256, 20), (10, 256), (7, 33)]            # (K, N)
    probs, refs, outs = [], [], []
    for q, (K, N) in enumerate(shapes):
        x, dy = _rand(M, K, seed=10 + q), _rand(M, N, seed=30 + q)
        dw, db = full(N, K), full(N)
        probs.append((ptr(dev(x)), ptr(dev(dy)), ptr(dw), ptr(db), M, K, N))
        refs.append((dy.double().t() @ x.double(), dy.double().sum(0)))
        outs.append((dw, db))
    arr, addr = _lib.wgrad_descs(probs)
    call("dvae_linear_wgrad_grouped", addr, len(probs), stream())
    for q, ((dw, db), (rw, rb)) in enumerate(zip(outs, refs)):
        check(dw, rw, what="grouped wgrad dw[%d] M=%d" % (q, M), **KTOL)
        check(db, rb, what="grouped wgrad db[%d] M=%d" % (q, M), **KTOL)


# ---- linears: the switches behind try_fc32 / try_gdma (use_small, pick_split, the split-contraction grids, try_gdma's minima) ----
@pytest.mark.parametrize("M,K,N", [(40, 4096, 36), (40, 4100, 36), (6080, 516, 100), (6081, 516, 100)])
def test_linear_forward_at_the_small_kernel_limits(M, K, N):
    """use_small (linear.hip): k_gemm32<true, true> takes an aligned forward of < 192 output tiles of 64x64 (95 x 2 | 96 x 2)
    with a contraction of at most 4096 (4096 | 4100); beyond either, k_gemm<true, false>."""
    _linear(M, K, N, act=_lib.ACT_LEAKY02, parts=("fwd",))


@pytest.mark.parametrize("M,K,N,parts", [(40, 127, 36, ("fwd",)), (40, 129, 36, ("fwd",)), (40, 1023, 36, ("fwd",)),
                                         (40, 1025, 36, ("fwd",)), (40, 2049, 36, ("fwd",)),
                                         (1024, 129, 960, ("fwd",)), (1024, 129, 1024, ("fwd",)),
                                         (127, 513, 512, ("wgrad",)), (129, 513, 512, ("wgrad",)),
                                         (40, 36, 1025, ("dgrad",))])
def test_linear_at_the_contraction_slice_switches(M, K, N, parts):
    """pick_split and the weight gradient's own loop (linear.hip): S doubles while tiles * S < 256 and Kc / (2 S) >= 64, up to
    16.  One tile: S = 1 | 2 at Kc = 127 | 129, 8 | 16 at 1023 | 1025, 16 (the cap) at 2049; Kc = 129 over 240 | 256 tiles:
    S = 2 | 1; the weight gradient over M = 127 | 129 rows; the input gradient over N = 1025.  Without the workspace S = 1."""
    _linear(M, K, N, act=_lib.ACT_LEAKY02, parts=parts)


@pytest.mark.parametrize("M,K,N,parts", [(512, 301, 512, ("fwd",)), (512, 301, 516, ("fwd",)),
                                         (512, 512, 301, ("dgrad",)), (512, 516, 301, ("dgrad",)),
                                         (300, 511, 512, ("wgrad",)), (300, 513, 512, ("wgrad",))])
def test_linear_split_contraction_at_the_reduction_grid_cap(M, K, N, parts):
    """k_splitk_epilogue / k_splitk_reduce run min(ceil(n / 256), 1024) workgroups over the n output elements: 1024 | 1032
    (forward, input gradient: 512 x 512 | 512 x 516) and 1022 | 1026 (weight gradient: 512 x 511 | 512 x 513) wanted."""
    _linear(M, K, N, act=_lib.ACT_LEAKY02, parts=parts)


@pytest.mark.parametrize("M,K,N,parts", [(2048, 252, 1024, ("fwd",)), (2048, 256, 1024, ("fwd",)),
                                         (40, 516, 124, ("fwd",)), (40, 516, 128, ("fwd",)),
                                         (40, 124, 516, ("dgrad",)), (40, 128, 516, ("dgrad",)),
                                         (100, 960, 512, ("wgrad",)), (100, 1024, 512, ("wgrad",))])
def test_linear_at_the_dma_kernel_minima(M, K, N, parts):
    """try_gdma (gemm_dma.hip) takes contractions from 256 (252 | 256 at 512 output tiles, where try_fc32 has declined) into
    at least 128 columns (124 | 128); try_gdma_wgrad takes outputs of at least 128 tiles of 64x64 (8 x 15 | 8 x 16)."""
    _linear(M, K, N, act=_lib.ACT_LEAKY02, parts=parts)


@pytest.mark.parametrize("M", [16384, 16388])
def test_narrow_input_gradient_at_its_grid_cap(M):
    """k_narrow_out_dgrad: min(ceil(M * K / 4 / 256), 4096) workgroups -- 4096 | 4097 wanted at K = 256."""
    _linear(M, 256, 2, act=_lib.ACT_NONE, parts=("dgrad",))


# ---- element-wise kernels: the grid caps of loss.hip --------------------------------------------------------------------------
@pytest.mark.parametrize("over", [0, 1])
def test_elementwise_kernels_at_their_grid_caps(over):
    """k_sigmoid_bwd (4096 workgroups of 256 elements), k_add and k_axpby (2048), k_u8_to_f32 (4096 of 256 x 16 bytes): the
    last size that the grid covers in one trip and the first at which the grid-stride loop takes a second."""
    g = torch.Generator().manual_seed(5 + over)
    n = 4096 * 256 + over
    gy, y = torch.randn(n, generator=g), torch.rand(n, generator=g)
    out = full(n)
    call("dvae_sigmoid_bwd", ptr(dev(gy)), ptr(dev(y)), ptr(out), n, stream())
    check(out, gy.double() * y.double() * (1 - y.double()), rtol=1e-4, atol_rel=1e-6, what="sigmoid bwd n=%d" % n)
    n = 2048 * 256 + over
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    ad, bd, out = dev(a), dev(b), full(n)
    call("dvae_add", ptr(ad), ptr(bd), ptr(out), n, stream())
    assert torch.equal(out.cpu(), (a.double() + b.double()).float()), "add n=%d" % n
    out = full(n)
    call("dvae_axpby", ptr(out), ptr(ad), 0.125, ptr(bd), 7.0, n, stream())
    torch.testing.assert_close(out.cpu(), (0.125 * a.double() + 7.0 * b.double()).float(), rtol=2e-7, atol=1e-6)
    n = 4096 * 256 * 16 + 16 * over
    u8 = torch.randint(0, 256, (n,), dtype=torch.uint8, generator=g)
    out = full(n)
    call("dvae_u8_to_f32", ptr(u8.to(DEV)), ptr(out), n, stream())
    assert torch.equal(out.cpu(), u8.to(torch.float32).div(255)), "u8_to_f32 n=%d" % n


# ---- convT3 on the staged records, 3 channels, buffers that the matrix-core kernel declines -----------------------------------
_ALL_FALLBACK_COMBOS = tuple((dist, is_u8) for dist in (0, 1, 2) for is_u8 in (0, 1))


def _convT3_staged_fallback(N, combos=_ALL_FALLBACK_COMBOS):
    """dvae_convT3_fwd_staged at C = 3 on buffers k_up_thin_mm declines: the plain forward, then one fused launch per
    (distribution, uint8 target) of `combos`; every unused partial slot (index >= the grid of min(8 N, 1536) workgroups) must
    read 0.0 after a 7.0 pre-fill."""
    C = 3
    w, b = _rand(32, C, 4, 4, seed=2, scale=0.2), _rand(C, seed=3, scale=0.1)
    wd, bd = dev(w), dev(b)
    pairs = torch.full((32 * _lib.thin_pair_floats(C),), 7.0, device=DEV)
    _stage(thin=(wd, pairs, C))
    xs = torch.relu(_rand(N, 32, 32, 32, seed=1))
    x = nhwc(xs)
    tgt8 = torch.randint(0, 256, (N, C, 64, 64), dtype=torch.uint8, generator=torch.Generator().manual_seed(4))
    tgt = tgt8.float() / 255.0
    coef = torch.zeros(_lib.NCOEF); coef[_lib.C_INV_B] = 1.0 / N
    coefd = dev(coef)
    numel = N * C * 64 * 64

    def off8():                                      # numel floats, 8 bytes into a 7.0-filled arena
        arena = full(numel + 2)
        v = arena[2:]
        assert ptr(v) % 16 == 8
        return arena, v

    t32a, t32 = off8()
    t32.copy_(tgt.reshape(-1))
    t8a = torch.zeros(numel + 2, dtype=torch.uint8, device=DEV)
    t8 = t8a[2:]
    t8.copy_(tgt8.reshape(-1))
    assert ptr(x) % 16 == 0 and ptr(t8) % 4 == 2
    logit = F.conv_transpose2d(xs.double(), w.double(), b.double(), stride=2, padding=1)
    pr, t64 = torch.sigmoid(logit), tgt.double()
    tol = dict(rtol=1e-5, atol_rel=2e-6)
    ra, r = off8()
    call("dvae_convT3_fwd_staged", ptr(x), ptr(pairs), ptr(bd), None, 0, ptr(r), None, 0, None, None, N, C, stream())
    check(r, pr.reshape(-1), what="fallback convT3 fwd", **tol)
    assert torch.all(ra[:2] == 7.0)
    grid = min(8 * N, 1536)                                   # launch_up_thin_staged (conv_thin.hip)
    for dist in (0, 1, 2):
        if dist == 0:
            tot = F.binary_cross_entropy(pr, t64, reduction="sum"); gref = (pr - t64) / N
        elif dist == 1:
            tot = ((255 * pr - 255 * t64) ** 2).sum() / 255; gref = 2 * 255 * (pr - t64) * pr * (1 - pr) / N
        else:
            tot = 3 * (pr - t64).abs().sum(); gref = 3 * torch.sign(pr - t64) * pr * (1 - pr) / N
        for tp, is_u8, nm in ((t32, 0, "fp32"), (t8, 1, "uint8")):
            if (dist, is_u8) not in combos:
                continue
            ra, r = off8()
            ga, gg = off8()
            part = torch.full((_lib.REC_NPART,), 7.0, device=DEV)
            call("dvae_convT3_fwd_staged", ptr(x), ptr(pairs), ptr(bd), ptr(tp), is_u8, ptr(r), ptr(gg), dist, ptr(coefd),
                 ptr(part), N, C, stream())
            tag = "fallback convT3 N=%d %s target dist %d " % (N, nm, dist)
            check(r, pr.reshape(-1), what=tag + "recon", **tol)
            check(part.sum(), tot, rtol=1e-5, what=tag + "loss sum")
            check(gg, gref.reshape(-1), rtol=1e-4, atol_rel=4e-6, what=tag + "dL/dlogit")
            assert torch.all(ra[:2] == 7.0) and torch.all(ga[:2] == 7.0), tag + "the floats in front are untouched"
            assert torch.all(part[grid:] == 0.0), tag + "unused partial slots read as zero"


def test_convT3_staged_falls_back_to_the_packed_fma_kernel():
    """dvae_convT3_fwd_staged at C = 3 runs k_up_thin_mm only on 16-byte aligned recon / g / fp32 target and a 4-byte aligned
    uint8 target; here recon, g and the fp32 target are views 8 bytes into their arenas and the uint8 target 2 bytes into its
    (the float2 / uchar2 accesses of k_up_thin_pk<3, *> stay naturally aligned), so all three instantiations of the fallback
    run: reconstruction, dL/dlogit and the likelihood sum against fp64 at the tolerances of
    test_convT3_forward_on_staged_pair_records."""
    _convT3_staged_fallback(3)


def test_convT3_staged_fallback_past_its_grid_cap():
    """The same fall-back at 193 images: 1544 units on the 1536 workgroups of k_up_thin_pk<3, *> (launch_up_thin_staged), so
    workgroups 0, 8, .. 56 (the XCD-aware unit map is on: the grid is a multiple of 64) take a second unit.  One launch without
    a target and one per distribution, fp32 and uint8 targets in turn."""
    _convT3_staged_fallback(193, combos=((0, 0), (1, 1), (2, 0)))


# ---- Adam: the by-value table holds ADAM_MAX_T = 64 tensors per launch --------------------------------------------------------
def _ulp(a, b):
    return ((a - b).abs() / (b.abs() * 2.0 ** -23 + 1e-9)).max().item()


@pytest.mark.parametrize("nt", [64, 65])
def test_adam_at_the_table_split(nt):
    """dvae_adam_step over 64 tensors (one launch) and 65 (two: the last tensor, 4097 elements = two workgroups, alone in the
    second), tensors of 4095 / 4096 / 4097 / 1 elements among them (ADAM_CHUNK = 4096), every buffer 4 bytes into its arena
    (the scalar path), two steps against torch's CPU Adam on the same gradients: parameters <= 1 ulp, state as
    test_gpu_adam.py holds it."""
    lr, betas, eps, wd = 5e-4, (0.9, 0.999), 1e-8, 0.0
    g = torch.Generator().manual_seed(nt)
    sizes = [int(s) for s in torch.randint(2, 300, (nt - 4,), generator=g)] + [4095, 4096, 1, 4097]
    total = sum(sizes)
    cpu = []
    for n in sizes:
        cpu.append(torch.nn.Parameter(torch.randn(n, generator=g)))
    oc = torch.optim.Adam(cpu, lr=lr, betas=betas, eps=eps, weight_decay=wd)
    arena = {k: torch.zeros(total + 1, device=DEV) for k in "pgmv"}
    steps = torch.zeros(nt, device=DEV)
    view, off = [], 1
    for n in sizes:
        view.append({k: arena[k][off:off + n] for k in "pgmv"})
        off += n
    for pc, v in zip(cpu, view):
        v["p"].copy_(pc.detach())
    tab = (_lib.AdamTensor * nt)()
    for i, (e, v, n) in enumerate(zip(tab, view, sizes)):
        e.p, e.g, e.m, e.v, e.step, e.n = ptr(v["p"]), ptr(v["g"]), ptr(v["m"]), ptr(v["v"]), steps.data_ptr() + 4 * i, n
    assert all(ptr(view[0][k]) % 16 == 4 for k in "pgmv")
    for step in (1, 2):
        for pc, v in zip(cpu, view):
            gr = torch.randn(pc.shape, generator=g) * (10.0 ** (step - 1))
            pc.grad = gr.clone()
            v["g"].copy_(gr)
        oc.step()
        call("dvae_adam_step", ctypes.addressof(tab), nt, float(step), lr, betas[0], betas[1], eps, wd, stream())
        torch.cuda.synchronize()
        assert torch.equal(steps.cpu(), torch.full((nt,), float(step)))
        for k, (pc, v) in enumerate(zip(cpu, view)):
            d = _ulp(v["p"].cpu(), pc.detach())
            assert d <= 1.0, "step %d tensor %d (%d elements): %.2f ulp" % (step, k, sizes[k], d)
            sc = oc.state[pc]
            assert float(sc["step"]) == step
            check(v["m"], sc["exp_avg"], rtol=1e-6, atol_rel=1e-7, what="exp_avg %d" % k)
            check(v["v"], sc["exp_avg_sq"], rtol=1e-6, atol_rel=1e-7, what="exp_avg_sq %d" % k)
        for pc, v in zip(cpu, view):               # re-synchronise: the comparison stays a one-step one
            v["p"].copy_(pc.detach())
    assert float(arena["p"][0]) == 0.0 and all(float(arena[k][0]) == 0.0 for k in "gmv")      # the pad in front is untouched
