"""-m gpu: parity at the persistent-grid caps and pipeline trip counts that tests/test_gpu_kernel_variants.py leaves out
(tests/kernel_variants.py: the rest of SWITCHES, and TRIP_CLASSES).  A persistent kernel's grid stops growing with the batch at a
cap; from there a workgroup takes a second trip through its loop, and in the software-pipelined loops the trip count meets the
depth of an LDS ring, its parity picks an output stage, and neighbouring workgroups of one launch differ by one trip.  Same
pattern as the sibling file: one or a few C-ABI calls on seeded inputs, outputs pre-filled with 7.0, an fp64 torch-CPU reference
of the same operation.  No tolerance is new: KTOL (rtol 1e-5 + 2e-6 max|ref|) for the tuned conv kernels, check()'s default
for the shape-generic ones, the bounds of test_convT3_forward_on_staged_pair_records / test_convT_sigmoid_recon_fused for the
likelihood, of test_recon_rows_vs_fp64_oracle for dvae_recon_rows, <= 1 ulp of torch's CPU Adam for Adam."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from gpu_util import *  # noqa
from gpu_util import _lib  # noqa
from oracle import disvae_oracle as O
from test_gpu_fused_core import _rand, _stage
from test_gpu_kernel_variants import KTOL, full, _ws, _wgrad32, _ulp
from test_gpu_loglik import recon_rows, images, as_f64

DISTS = ("bernoulli", "gaussian", "laplace")
NPART = _lib.REC_NPART


def _likelihood_refs(pr, t64, dist, N):
    """fp64 likelihood sum over the batch and dL/dlogit of the mean (losses.py:394-449 behind the sigmoid), dist = 0 / 1 / 2."""
    if dist == 0:
        return F.binary_cross_entropy(pr, t64, reduction="sum"), (pr - t64) / N
    if dist == 1:
        return ((255 * pr - 255 * t64) ** 2).sum() / 255, 2 * 255 * (pr - t64) * pr * (1 - pr) / N
    return 3 * (pr - t64).abs().sum(), 3 * torch.sign(pr - t64) * pr * (1 - pr) / N


def _check_dlogit(gl, gref, pr, t64, dist, what):
    """dL/dlogit against fp64 at rtol 1e-4 + 4e-6 max|ref| (test_convT3_forward_on_staged_pair_records).  The Laplace term's
    derivative 3 sign(p - t) jumps at p = t, and these cases have millions of elements: where the fp64 reconstruction lies
    within the reconstruction's own tolerance (KTOL, asserted beside this check) of the target, a correct fp32 reconstruction
    may sit on the other side of it, or ON it (sign = 0: the kernel's p equals the fp32 target) -- there the kernel's value is
    held to the three values sign() can take, everywhere else to the reference."""
    got = gl.detach().cpu().double().reshape(gref.shape)
    if dist == 2:
        near = (pr - t64).abs() <= KTOL["rtol"] * pr.abs() + KTOL["atol_rel"] * pr.abs().max()
        assert int(near.sum()) <= 1e-4 * near.numel(), what + ": %d elements at the kink" % int(near.sum())
        g3 = gref[near].abs()                                         # = 3 p (1 - p) / N
        off = torch.minimum((got[near].abs() - g3).abs(), got[near].abs())
        assert torch.all(off <= 1e-4 * g3 + 4e-6 * gref.abs().max()), what + ": neither +-3 p (1 - p) / N nor 0 at p = target"
        got = torch.where(near, gref, got)
    check(got, gref, rtol=1e-4, atol_rel=4e-6, what=what)


def _parts():
    return torch.full((NPART,), 7.0, device=DEV)


def _coef(N):
    coef = torch.zeros(_lib.NCOEF)
    coef[_lib.C_INV_B] = 1.0 / N
    return dev(coef)


# ---- uint8 entry points of the thin ends against fp64 (the bit-for-bit test of test_gpu_uint8_input.py compares two
# ---- instantiations of one template: a mistake both share passes it) -----------------------------------------------------------
@pytest.mark.parametrize("N,C,dist", [(64, 3, 0), (65, 1, 1), (128, 3, 2), (192, 1, 0), (193, 1, 1), (193, 3, 2), (256, 3, 0),
                                      (384, 3, 1), (576, 1, 0), (768, 1, 1)])
def test_u8_thin_kernels_vs_fp64(N, C, dist):
    """dvae_conv4s2_fwd_u8, dvae_conv4s2_wgrad_u8 and dvae_convT4s2_sigmoid_recon_fwd_u8 on a uint8 image against fp64 on
    ToTensor(image).  Units = 8 N; k_down_thin<C, 0, uint8> and k_up_thin<C, true, uint8> run min(8 N, 1536) workgroups,
    k_wgrad_thin<C, uint8> min(8 N, WT_MAX_BLOCKS = 512):
      N = 64 | 65: the weight gradient's cap (1 | 2 trips);  128 / 192 / 256: 2 / 3 / 4 trips in each of its workgroups;
      N = 192 | 193: the cap of the other two (193: workgroups of image 0 take a second unit);
      N = 384 / 576 / 768: 2 / 3 / 4 trips in every workgroup of the forward and the fused likelihood (6 / 9 / 12 of the
      weight gradient): k_down_thin keeps two tiles in flight in registers and is unrolled by two trips."""
    tag = "u8 thin N=%d C=%d " % (N, C)
    g = torch.Generator().manual_seed(N + C)
    u8 = torch.randint(0, 256, (N, C, 64, 64), dtype=torch.uint8, generator=g)
    x64 = u8.double() / 255
    ud = keep(u8.to(DEV))
    w, b = _rand(32, C, 4, 4, seed=2, scale=0.2), _rand(32, seed=3, scale=0.1)
    wr, br = w.double().requires_grad_(True), b.double().requires_grad_(True)
    pre = F.conv2d(x64, wr, br, stride=2, padding=1)
    y = full(N, 32, 32, 32)
    call("dvae_conv4s2_fwd_u8", ptr(ud), ptr(dev(w)), ptr(dev(b)), ptr(y), N, C, 64, 64, 32, _lib.ACT_RELU, stream())
    check(from_nhwc(y, N, 32, 32, 32), torch.relu(pre).detach(), what=tag + "conv1 fwd", **KTOL)
    dy = _rand(N, 32, 32, 32, seed=4)                         # NCHW values
    pre.backward(dy.double())
    dw, db = full(32, C, 4, 4), full(32)
    call("dvae_conv4s2_wgrad_u8", ptr(ud), ptr(nhwc(dy)), ptr(dw), ptr(db), N, C, 64, 64, 32, ptr(_ws()), stream())
    check(dw, wr.grad, what=tag + "conv1 wgrad", **KTOL)
    check(db, br.grad, what=tag + "conv1 bias grad", **KTOL)
    # fused last decoder layer: the target is the uint8 image
    a = torch.relu(_rand(N, 32, 32, 32, seed=5))
    wt, bt = _rand(32, C, 4, 4, seed=6, scale=0.2), _rand(C, seed=7, scale=0.1)
    recon, gl, parts = full(N, C, 64, 64), full(N, C, 64, 64), _parts()
    call("dvae_convT4s2_sigmoid_recon_fwd_u8", ptr(nhwc(a)), ptr(dev(wt)), ptr(dev(bt)), ptr(ud), ptr(recon), ptr(gl), dist,
         ptr(_coef(N)), ptr(parts), N, 32, 32, 32, C, stream())
    pr = torch.sigmoid(F.conv_transpose2d(a.double(), wt.double(), bt.double(), stride=2, padding=1))
    tot, gref = _likelihood_refs(pr, x64, dist, N)
    check(recon, pr, what=tag + "fused recon", **KTOL)
    check(parts.sum(), tot, rtol=1e-5, what=tag + "fused loss sum")
    _check_dlogit(gl, gref, pr, x64, dist, tag + "fused dL/dlogit")
    assert torch.all(parts[min(8 * N, 1536):] == 0.0), tag + "unused partial slots read as zero"


# ---- fused convT3 + likelihood: k_up_thin<C, true, T> runs min(8 N, 1536) workgroups of one unit per trip ------------------------
@pytest.mark.parametrize("N,C,dist,u8", [(192, 1, 0, False), (193, 1, 1, False), (192, 3, 2, False), (193, 3, 0, False),
                                         (192, 1, 1, True), (193, 1, 2, True), (192, 3, 0, True), (193, 3, 1, True),
                                         (8, 3, 2, False), (9, 1, 0, True), (8, 1, 1, True), (9, 3, 2, False)])
def test_fused_convT3_likelihood_at_the_grid_cap(N, C, dist, u8):
    """dvae_convT4s2_sigmoid_recon_fwd / _u8 at 192 | 193 images (launch_up_thin_recon / _u8: 1536 | 1544 units on at most 1536
    workgroups), every distribution on either side: reconstruction and dL/dlogit against fp64, the sum over all
    DVAE_REC_NPART partial slots against the fp64 loss at test_convT_sigmoid_recon_fused's bound, and every slot from the grid
    size on exactly 0.0 after a 7.0 pre-fill (the zeroing loop starts at gridDim.x).
    8 | 9 images: the XCD-aware unit map is on when the grid is a multiple of 64 and off otherwise; of the existing cases the
    small ones (3, 4, 5 images: 24, 32, 40 workgroups) have it off and the large ones (263, 300, 1024 images: 1536) on with
    more than one trip -- 8 images are the map on a single-trip grid, 9 the first grid above it without."""
    tag = "fused convT3 N=%d C=%d dist %d%s " % (N, C, dist, " u8" if u8 else "")
    a = torch.relu(_rand(N, 32, 32, 32, seed=1))
    w, b = _rand(32, C, 4, 4, seed=2, scale=0.2), _rand(C, seed=3, scale=0.1)
    g = torch.Generator().manual_seed(4)
    if u8:
        t8 = torch.randint(0, 256, (N, C, 64, 64), dtype=torch.uint8, generator=g)
        t64, td = t8.double() / 255, keep(t8.to(DEV))
    else:
        t32 = torch.rand(N, C, 64, 64, generator=g)
        t64, td = t32.double(), dev(t32)
    recon, gl, parts = full(N, C, 64, 64), full(N, C, 64, 64), _parts()
    if u8:
        call("dvae_convT4s2_sigmoid_recon_fwd_u8", ptr(nhwc(a)), ptr(dev(w)), ptr(dev(b)), ptr(td), ptr(recon), ptr(gl), dist,
             ptr(_coef(N)), ptr(parts), N, 32, 32, 32, C, stream())
    else:
        call("dvae_convT4s2_sigmoid_recon_fwd", ptr(nhwc(a)), _lib.NHWC, ptr(dev(w)), ptr(dev(b)), ptr(td), ptr(recon), ptr(gl),
             dist, ptr(_coef(N)), ptr(parts), N, 32, 32, 32, C, stream())
    pr = torch.sigmoid(F.conv_transpose2d(a.double(), w.double(), b.double(), stride=2, padding=1))
    tot, gref = _likelihood_refs(pr, t64, dist, N)
    assert abs(O.reconstruction_loss(t64, pr, DISTS[dist]).item() - tot.item() / N) <= 1e-12 * abs(tot.item())
    check(recon, pr, what=tag + "recon", **KTOL)
    check(parts.sum() / N, tot / N, rtol=2e-5, what=tag + "loss")
    _check_dlogit(gl, gref, pr, t64, dist, tag + "dL/dlogit")
    assert torch.all(parts[min(8 * N, 1536):] == 0.0), tag + "unused partial slots read as zero"


# ---- staged convT3 forward: k_up_thin_mm (C = 3) min(3 N, 512) workgroups, k_up_thin_pk (C = 1) min(8 N, 1536) ------------------
@pytest.mark.parametrize("N,C", [(170, 3), (171, 3), (192, 1), (193, 1), (384, 1), (512, 3), (576, 1), (1024, 3)])
def test_staged_convT3_at_the_grid_caps(N, C):
    """dvae_convT3_fwd_staged without a target, with an fp32 and with a uint8 target (the distributions rotate over the cases)
    against fp64 at the bounds of test_convT3_forward_on_staged_pair_records; unused partial slots read 0.0 after a 7.0
    pre-fill (k_up_thin_mm's zeroing loop strides by 512 threads, k_up_thin_pk's by 128).
      C = 3, k_up_thin_mm: 3 N units on at most 512 workgroups -- 170 | 171 images are 510 | 513 units; 512 and 1024 images are
      3 and 6 trips in every workgroup (3 N is a multiple of 512 only then: no image count gives 2), the next tile travels in
      registers under the current one.
      C = 1, k_up_thin_pk: 8 N units on at most 1536 workgroups -- 192 | 193 images; 384 and 576 are 2 and 3 trips everywhere."""
    tag = "staged convT3 N=%d C=%d " % (N, C)
    w, b = _rand(32, C, 4, 4, seed=2, scale=0.2), _rand(C, seed=3, scale=0.1)
    wd, bd = dev(w), dev(b)
    pairs = torch.full((32 * _lib.thin_pair_floats(C),), 7.0, device=DEV)
    _stage(thin=(wd, pairs, C))
    xs = torch.relu(_rand(N, 32, 32, 32, seed=1))
    x = nhwc(xs)
    t8 = torch.randint(0, 256, (N, C, 64, 64), dtype=torch.uint8, generator=torch.Generator().manual_seed(4))
    t32 = t8.float() / 255.0
    t64 = t32.double()
    pr = torch.sigmoid(F.conv_transpose2d(xs.double(), w.double(), b.double(), stride=2, padding=1))
    tol = dict(rtol=1e-5, atol_rel=2e-6)
    grid = min(3 * N, 512) if C == 3 else min(8 * N, 1536)
    r = full(N, C, 64, 64)
    call("dvae_convT3_fwd_staged", ptr(x), ptr(pairs), ptr(bd), None, 0, ptr(r), None, 0, None, None, N, C, stream())
    check(r, pr, what=tag + "fwd", **tol)
    coefd = _coef(N)
    d32 = (N + C) % 3
    for tp, is_u8, dist in ((dev(t32), 0, d32), (keep(t8.to(DEV)), 1, (d32 + 1) % 3)):
        r, gg, part = full(N, C, 64, 64), full(N, C, 64, 64), _parts()
        call("dvae_convT3_fwd_staged", ptr(x), ptr(pairs), ptr(bd), ptr(tp), is_u8, ptr(r), ptr(gg), dist, ptr(coefd), ptr(part),
             N, C, stream())
        tot, gref = _likelihood_refs(pr, t64, dist, N)
        t = tag + "%s target dist %d " % ("uint8" if is_u8 else "fp32", dist)
        check(r, pr, what=t + "recon", **tol)
        check(part.sum(), tot, rtol=1e-5, what=t + "loss sum")
        _check_dlogit(gg, gref, pr, t64, dist, t + "dL/dlogit")
        assert torch.all(part[grid:] == 0.0), t + "unused partial slots read as zero"


# ---- 32 <-> 32 channel weight gradients ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("small_nchw", [False, True])
@pytest.mark.parametrize("N", [1024, 1025])
def test_wgrad32_4x4_at_the_grid_cap(N, small_nchw, transposed):
    """k_wgrad32<4>: ceil(N / 4) units on at most WG_MAX_BLOCKS = 256 workgroups (launch_wgrad_t, conv_mfma.hip) -- 1024 | 1025
    images, conv and convT, the 4x4 side NHWC and NCHW."""
    _wgrad32(N, 4, transposed, small_nchw)


@pytest.mark.parametrize("N", [2048, 3072, 4096])
def test_wgrad32_4x4_trip_counts(N):
    """k_wgrad32<4> prefetches the next unit into registers under the current one: 2, 3 and 4 trips in every workgroup
    (test_4x4_end_nchw_persistent of test_gpu_bench_sizes.py runs 1 and 5 | 4)."""
    _wgrad32(N, 4, transposed=False)


@pytest.mark.parametrize("N", [64, 144, 192, 240, 288])
def test_wgrad32ws_trip_counts(N):
    """k_wgrad32ws<16>: 4 N units; 256 workgroups up to 128 images, 192 for 128 < N <= 320 (launch_wgrad_ws_t).  A unit is
    multiplied while the next sits in the second LDS buffer and the two after it in the register sets A / B, the loop unrolled
    by two: 64 images are 1 trip in every workgroup, 144 / 192 / 240 / 288 are 3 / 4 / 5 / 6
    (test_conv_wgrad32_at_the_grid_cap: 128 images = 2 trips, 129 = 3 | 2)."""
    _wgrad32(N, 16, transposed=False)


# ---- shape-generic conv kernels: grid_for caps the grid at 8192 workgroups of 256 threads ------------------------------------------
def _generic_down(N, Cb, Cs, Hs):
    """Conv2d forward (bias + ReLU) and ConvTranspose2d input gradient (masked) big[N, Cb, 2 Hs, 2 Hs] NCHW -> small NHWC."""
    Hb = 2 * Hs
    tag = "generic down N=%d %d->%d Hs=%d " % (N, Cb, Cs, Hs)
    x = _rand(N, Cb, Hb, Hb, seed=1)
    w, b = _rand(Cs, Cb, 4, 4, seed=2, scale=0.2), _rand(Cs, seed=3, scale=0.1)
    xd, wd = dev(x), dev(w)
    y = full(N, Hs, Hs, Cs)
    call("dvae_conv4s2_fwd", ptr(xd), _lib.NCHW, ptr(wd), ptr(dev(b)), ptr(y), _lib.NHWC, N, Cb, Hb, Hb, Cs, _lib.ACT_RELU, stream())
    down = F.conv2d(x.double(), w.double(), None, stride=2, padding=1)
    check(from_nhwc(y, N, Cs, Hs, Hs), torch.relu(down + b.double().view(1, Cs, 1, 1)), what=tag + "conv fwd")
    act = torch.relu(_rand(N, Cs, Hs, Hs, seed=5))
    dx = full(N, Hs, Hs, Cs)
    call("dvae_convT4s2_dgrad", ptr(xd), _lib.NCHW, ptr(wd), ptr(nhwc(act)), ptr(dx), _lib.NHWC, N, Cs, Hs, Hs, Cb, stream())
    check(from_nhwc(dx, N, Cs, Hs, Hs), down * (act > 0), what=tag + "convT dgrad")


def _generic_up(N, Cb, Cs, Hs):
    """ConvTranspose2d forward (bias + sigmoid) and Conv2d input gradient (masked) small[N, Hs, Hs, Cs] NHWC -> big NCHW."""
    Hb = 2 * Hs
    tag = "generic up N=%d %d->%d Hs=%d " % (N, Cs, Cb, Hs)
    s = _rand(N, Cs, Hs, Hs, seed=1)
    w, b = _rand(Cs, Cb, 4, 4, seed=2, scale=0.2), _rand(Cb, seed=3, scale=0.1)
    sd, wd = nhwc(s), dev(w)
    y = full(N, Cb, Hb, Hb)
    call("dvae_convT4s2_fwd", ptr(sd), _lib.NHWC, ptr(wd), ptr(dev(b)), ptr(y), _lib.NCHW, N, Cs, Hs, Hs, Cb, _lib.ACT_SIGMOID, stream())
    up = F.conv_transpose2d(s.double(), w.double(), None, stride=2, padding=1)
    check(y, torch.sigmoid(up + b.double().view(1, Cb, 1, 1)), what=tag + "convT fwd")
    act = torch.relu(_rand(N, Cb, Hb, Hb, seed=5))
    dx = full(N, Cb, Hb, Hb)
    call("dvae_conv4s2_dgrad", ptr(sd), _lib.NHWC, ptr(wd), ptr(dev(act)), ptr(dx), _lib.NCHW, N, Cb, Hb, Hb, Cs, stream())
    check(dx, up * (act > 0), what=tag + "conv dgrad")


# (kernel, direction, N at 8192 workgroups, Cb, Cs, Hs): total / 256 workgroups wanted, total as the launcher counts it
GENERIC_GRID = {
    "down_thin_px1": (_generic_down, 16384, 1, 32, 4),       # N * Hs * Ws * 8 threads:          N / 2 workgroups
    "down_thin_px3": (_generic_down, 16384, 3, 32, 4),
    "down_generic": (_generic_down, 8192, 2, 16, 4),         # N * Cs * Hs * Ws = 256 N threads:  N workgroups
    "up_thin_px1": (_generic_up, 8192, 1, 32, 8),            # N * Cb * 4 Hs Ws = 256 N threads:  N workgroups
    "up_thin_px3": (_generic_up, 10922, 3, 32, 4),           # 192 N threads: 8191.5 -> 8192 | 8192.25 -> 8193
    "up_generic": (_generic_up, 8192, 4, 2, 4),              # N * Cb * 4 Hs Ws = 256 N threads:  N workgroups
}


@pytest.mark.parametrize("over", [0, 1])
@pytest.mark.parametrize("kernel", sorted(GENERIC_GRID))
def test_generic_conv_at_the_grid_cap(kernel, over):
    """grid_for (conv_generic.hip) caps k_down_generic, k_up_generic, k_down_thin_px<C> and k_up_thin_px<C> at 8192 workgroups
    of 256 threads, behind which they stride: each kernel at the last image count that wants exactly 8192 workgroups and at the
    next one, which wants 8193 (the first 256 threads take a second element).  Forward and masked input gradient at check()'s
    default, as test_conv_fwd_dgrad_wgrad holds these kernels.  The thin-pixel kernels take Cs = 32 with Cb = 1 / 3 at any size
    but 64x64; 2 -> 16 and 2 -> 4 channels are geometries that no tuned kernel and neither of them takes."""
    fn, N, Cb, Cs, Hs = GENERIC_GRID[kernel]
    fn(N + over, Cb, Cs, Hs)


@pytest.mark.parametrize("N", [61, 62])
def test_generic_wgrad_at_the_workspace_switch(N):
    """launch_wgrad_generic takes the chunked pair k_wgrad_generic_part / _fin only while chunks * Cs * Cb * 17 floats fit the
    workspace of dvae_conv_wgrad_ws_floats() = 256 * 16704: with Cs = Cb = 64 and 32x32 small sides (chunks = N) 61 chunks
    fit (4 247 552 floats), 62 do not (4 317 184) and k_wgrad_generic + k_chansum run instead."""
    Cb = Cs = 64
    assert 61 * Cs * Cb * 17 <= _lib.lib().dvae_conv_wgrad_ws_floats() < 62 * Cs * Cb * 17
    x = _rand(N, Cb, 64, 64, seed=1)
    dy = _rand(N, Cs, 32, 32, seed=4)
    w = torch.zeros(Cs, Cb, 4, 4, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(Cs, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), w, b, stride=2, padding=1).backward(dy.double())
    dw, db = full(Cs, Cb, 4, 4), full(Cs)
    call("dvae_conv4s2_wgrad", ptr(dev(x)), _lib.NCHW, ptr(nhwc(dy)), _lib.NHWC, ptr(dw), ptr(db), N, Cb, 64, 64, Cs, ptr(_ws()), stream())
    check(dw, w.grad, what="generic wgrad 64->64 N=%d dw" % N)
    check(db, b.grad, what="generic wgrad 64->64 N=%d db" % N)


# ---- dvae_recon_rows: one column slice per 1024 elements of a row ------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 9])
@pytest.mark.parametrize("row_elems", [1024, 1028, 2048, 2052])
@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("dist", DISTS)
def test_recon_rows_at_the_slice_switches(dist, u8, row_elems, K):
    """launch_recon_rows: nslice = ceil(row_elems / 4 / 256) -- 1024 | 1028 elements are 1 | 2 slices (k_recon_rows_finish runs
    from two; the second slice has ONE live quad), 2048 | 2052 are 2 | 3; K = 9 samples span two chunks of RR_ROWS = 8 rows.
    Every row against the fp64 restatement at test_recon_rows_vs_fp64_oracle's bound."""
    n_img = 3
    target = images(n_img, (row_elems,), u8, seed=K).to(DEV)
    recon = torch.rand((n_img * K, row_elems), generator=torch.Generator().manual_seed(row_elems + K))
    recon[0, :4] = torch.tensor([0.0, 1.0, 1e-30, 1.0 - 2 ** -24])
    recon[-1, -4:] = torch.tensor([1.0 - 2 ** -24, 1e-30, 1.0, 0.0])          # the last quad of the last slice
    recon = recon.to(DEV)
    got = recon_rows(recon, target, K, dist)
    t64, r64 = as_f64(target.cpu()), recon.cpu().double()
    for r in range(n_img * K):
        want = O.reconstruction_loss(t64[r // K:r // K + 1], r64[r:r + 1], dist).item()
        assert abs(got[r].item() - want) <= 2e-6 * (abs(want) + 1.0), (r, got[r].item(), want)


# ---- Adam: ADAM_CHUNK = 4096 elements per workgroup ----------------------------------------------------------------------------
@pytest.mark.parametrize("over", [0, 1])
def test_adam_at_the_chunk_switch(over):
    """One optimizer whose tensors have 4096 and 8192 elements (1 and 2 workgroups of ADAM_CHUNK) | 4097 and 8193 (2 and 3: the
    last workgroup updates one element), each once 16-byte aligned (the 16-byte path; 4097 / 8193: its scalar tail) and once
    4 bytes in (the scalar path), an empty and a one-element tensor among them; two steps against torch's CPU Adam on the same
    gradients: parameters <= 1 ulp, exp_avg / exp_avg_sq as test_gpu_adam.py holds them, every tensor's step count written --
    the empty one's too -- and nothing outside a tensor touched."""
    lr, betas, eps, wd = 5e-4, (0.9, 0.999), 1e-8, 0.0
    g = torch.Generator().manual_seed(11 + over)
    sizes = [4096 + over, 0, 8192 + over, 1]
    layout = [(n, off) for off in (0, 1) for n in sizes]              # (elements, floats past a 16-byte boundary)
    nt = len(layout)
    cpu = [torch.nn.Parameter(torch.randn(n, generator=g)) for n, _ in layout]
    oc = torch.optim.Adam(cpu, lr=lr, betas=betas, eps=eps, weight_decay=wd)
    view = []
    for n, off in layout:
        arenas = {k: keep(torch.full((n + 8,), 3.0, device=DEV)) for k in "pgmv"}
        view.append({k: a[off:off + n] for k, a in arenas.items()})
        view[-1]["arenas"] = arenas
        assert all(ptr(arenas[k]) % 16 == 0 for k in "pgmv")
    steps = torch.zeros(nt, device=DEV)
    for pc, v in zip(cpu, view):
        v["p"].copy_(pc.detach())
        v["m"].zero_()
        v["v"].zero_()
    tab = (_lib.AdamTensor * nt)()
    for i, (e, v, (n, off)) in enumerate(zip(tab, view, layout)):
        e.p, e.g, e.m, e.v = (ptr(v["arenas"][k]) + 4 * off for k in "pgmv")
        e.step, e.n = steps.data_ptr() + 4 * i, n
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
            n, off = layout[k]
            sc = oc.state[pc]
            assert float(sc["step"]) == step
            if n:
                d = _ulp(v["p"].cpu(), pc.detach())
                assert d <= 1.0, "step %d tensor %d (%d elements, %d floats in): %.2f ulp" % (step, k, n, off, d)
                check(v["m"], sc["exp_avg"], rtol=1e-6, atol_rel=1e-7, what="exp_avg %d" % k)
                check(v["v"], sc["exp_avg_sq"], rtol=1e-6, atol_rel=1e-7, what="exp_avg_sq %d" % k)
            for key in "pgmv":                                         # nothing outside [off, off + n) is written
                a = v["arenas"][key]
                assert torch.all(a[:off] == 3.0) and torch.all(a[off + n:] == 3.0), (k, key)
        for pc, v in zip(cpu, view):                                   # re-synchronise: the comparison stays a one-step one
            v["p"].copy_(pc.detach())
