"""-m gpu: the conv and linear families OFF the model's shapes -- one test case per negated equality term of the launcher
conditions (tests/kernel_variants.py: PREDICATES), each against the fp64 torch operation on the CPU.

The launchers choose a tuned kernel by conjunctions of `Cb == 32`, `Hs == Ws`, `layout == NHWC`, `act in {none, relu}`, `K % 4`,
`(ptr & 15) == 0`, ...; every other test of the suite sits inside those conjunctions (or forces the generic kernels at the same
shapes, where an H/W swap cancels).  Here each term is negated alone: H != W in both orders, channel counts beside 32 and beside
1 / 3, every layout pair, the spatial sizes no tuned kernel has, the activations the tuned kernels decline, NULL for every
optional pointer, and every pointer 4 and 8 bytes into a 16-byte-aligned buffer (the alignment contract of include/dvae_hip.h:
such a call must reach a kernel whose accesses are 4 bytes wide).  Outputs are pre-filled with 7.0 and sit between guard
floats that must survive.  Tolerances: the `check` defaults (rtol 1e-4 + 2e-5 max|ref|) the other tests hold these entry points
to; the fused likelihood at the values of test_gpu_kernels.py::test_convT_sigmoid_recon_fused.

Wall time on one MI355X (measured): 280 tests in 4.6 s of pytest, 7.2 s for the process; the slowest test takes 1.0 s (the
first launch of the file), every other one under 0.1 s.
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import kernel_variants as KV
from gpu_util import DEV, call, check, stream
from gpu_util import _lib
from disvae_amd._lib import DvaeHipError
from oracle import disvae_oracle as O

SENTINEL = 7.0
PAD = 8                                     # guard floats on either side of every buffer (32 bytes: the alignment of the middle holds)
LAYOUT = {"NCHW": _lib.NCHW, "NHWC": _lib.NHWC}
ACT = {"none": _lib.ACT_NONE, "relu": _lib.ACT_RELU, "sigmoid": _lib.ACT_SIGMOID, "leaky": _lib.ACT_LEAKY02}
_LIVE = []                                  # device buffers of the running test (a freed one could be re-used before the launch)


@pytest.fixture(autouse=True)
def _release():
    yield
    del _LIVE[:]
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                # a device fault is sticky: nothing after it can run, so nothing after it is started
        pytest.exit("the device reported %s" % e, returncode=3)


def _rand(*shape, seed, scale=1.0):
    return (torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1) * scale


def _apply(pre, act):
    return {"none": pre, "relu": torch.relu(pre), "sigmoid": torch.sigmoid(pre), "leaky": F.leaky_relu(pre, 0.2)}[act]


class Buf:
    """`n` floats `off` bytes past a 16-byte boundary, between 2 * PAD guard floats."""

    def __init__(self, n, off=0):
        assert off % 4 == 0 and 0 <= off < 4 * PAD
        self.n, self.k = n, PAD + off // 4
        self.buf = torch.full((n + 2 * PAD + 4,), SENTINEL, device=DEV)
        assert self.buf.data_ptr() % 16 == 0
        self.view = self.buf[self.k:self.k + n]
        assert self.view.data_ptr() % 16 == off % 16
        _LIVE.append(self)

    @property
    def p(self):
        return self.view.data_ptr()

    def guards_intact(self):
        return bool((self.buf[:self.k] == SENTINEL).all()) and bool((self.buf[self.k + self.n:] == SENTINEL).all())

    def untouched(self):
        return bool((self.buf == SENTINEL).all())


def _in(t, off=0):
    """cpu tensor (already in the memory order wanted) -> device Buf."""
    b = Buf(t.numel(), off)
    b.view.copy_(t.contiguous().reshape(-1).float())
    return b


def _to_layout(t, layout):
    return t.permute(0, 2, 3, 1).contiguous() if layout == "NHWC" else t.contiguous()


def _from_layout(buf, layout, N, C, H, W):
    v = buf.view.cpu()
    return v.view(N, H, W, C).permute(0, 3, 1, 2) if layout == "NHWC" else v.view(N, C, H, W)


_WS = []


def _ws(off=0):
    n = _lib.lib().dvae_conv_wgrad_ws_floats()
    if not _WS:
        _WS.append(torch.empty(n + 2 * PAD, device=DEV))
        assert _WS[0].data_ptr() % 16 == 0
    v = _WS[0][PAD + off // 4:PAD + off // 4 + n]
    assert v.data_ptr() % 16 == off % 16
    return v.data_ptr()


# ---- the conv family ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _conv_ref(N, Cb, Cs, H, W):
    """fp32 inputs and fp64 results of both directions at big[N,Cb,H,W] <-> small[N,Cs,H/2,W/2] (computed once per geometry;
    never modified).  Every element is an independent draw: rows and columns of an image differ, so an H/W swap shows."""
    Hs, Ws = H // 2, W // 2
    r = dict(big=_rand(N, Cb, H, W, seed=1), small=_rand(N, Cs, Hs, Ws, seed=2), w=_rand(Cs, Cb, 4, 4, seed=3, scale=0.2),
             b_small=_rand(Cs, seed=4, scale=0.1), b_big=_rand(Cb, seed=5, scale=0.1), dy_small=_rand(N, Cs, Hs, Ws, seed=6),
             dy_big=_rand(N, Cb, H, W, seed=7), mask_big=torch.relu(_rand(N, Cb, H, W, seed=8)),
             mask_small=torch.relu(_rand(N, Cs, Hs, Ws, seed=9)))
    for with_bias in (True, False):
        x, w = r["big"].double().requires_grad_(True), r["w"].double().requires_grad_(True)
        b = r["b_small"].double().requires_grad_(True)
        pre = F.conv2d(x, w, b if with_bias else None, stride=2, padding=1)            # w[Cout = Cs, Cin = Cb, 4, 4]
        r["conv_pre", with_bias] = pre.detach()
        if with_bias:
            pre.backward(r["dy_small"].double())
            r["conv_dx"], r["conv_dw"], r["conv_db"] = x.grad, w.grad, b.grad
        x, w = r["small"].double().requires_grad_(True), r["w"].double().requires_grad_(True)
        b = r["b_big"].double().requires_grad_(True)
        pre = F.conv_transpose2d(x, w, b if with_bias else None, stride=2, padding=1)   # w[Cin = Cs, Cout = Cb, 4, 4]
        r["convT_pre", with_bias] = pre.detach()
        if with_bias:
            pre.backward(r["dy_big"].double())
            r["convT_dx"], r["convT_dw"], r["convT_db"] = x.grad, w.grad, b.grad
    return r


def _run_conv_family(c):
    N, Cb, Cs, H, W, bl, sl = c["N"], c["Cb"], c["Cs"], c["H"], c["W"], c["bl"], c["sl"]
    Hs, Ws = H // 2, W // 2
    BL, SL = LAYOUT[bl], LAYOUT[sl]
    r = _conv_ref(N, Cb, Cs, H, W)
    role, nbytes = c["off"] or (None, 0)
    off = lambda name: nbytes if role == name else 0
    null = c["null"]
    tag = KV.conv_id(c)
    big, small, w = _in(_to_layout(r["big"], bl), off("big")), _in(_to_layout(r["small"], sl), off("small")), _in(r["w"], off("w"))
    b_small = None if null == "b" else _in(r["b_small"], off("b"))
    b_big = None if null == "b" else _in(r["b_big"], off("b"))
    dy_small, dy_big = _in(_to_layout(r["dy_small"], sl), off("small")), _in(_to_layout(r["dy_big"], bl), off("big"))
    mask_big = None if null == "mask" else _in(_to_layout(r["mask_big"], bl), off("mask"))
    mask_small = None if null == "mask" else _in(_to_layout(r["mask_small"], sl), off("mask"))
    P = lambda x: None if x is None else x.p
    wsp = None if null == "ws" else _ws(off("ws"))
    outs = []

    def out(n, name):
        o = Buf(n, off(name))
        outs.append(o)
        return o

    # Conv2d: big -> small
    y = out(N * Cs * Hs * Ws, "small")
    call("dvae_conv4s2_fwd", big.p, BL, w.p, P(b_small), y.p, SL, N, Cb, H, W, Cs, ACT[c["act"]], stream())
    check(_from_layout(y, sl, N, Cs, Hs, Ws), _apply(r["conv_pre", null != "b"], c["act"]), what=tag + " conv fwd")
    dx = out(N * Cb * H * W, "big")
    call("dvae_conv4s2_dgrad", dy_small.p, SL, w.p, P(mask_big), dx.p, BL, N, Cb, H, W, Cs, stream())
    mult = 1.0 if null == "mask" else (r["mask_big"] > 0).double()
    check(_from_layout(dx, bl, N, Cb, H, W), r["conv_dx"] * mult, what=tag + " conv dgrad")
    dw, db = out(Cs * Cb * 16, "dw"), (None if null == "db" else out(Cs, "db"))
    call("dvae_conv4s2_wgrad", big.p, BL, dy_small.p, SL, dw.p, P(db), N, Cb, H, W, Cs, wsp, stream())
    check(dw.view.view(Cs, Cb, 4, 4), r["conv_dw"], what=tag + " conv wgrad")
    if db is not None:
        check(db.view, r["conv_db"], what=tag + " conv bias grad")
    # ConvTranspose2d: small -> big
    y = out(N * Cb * H * W, "big")
    call("dvae_convT4s2_fwd", small.p, SL, w.p, P(b_big), y.p, BL, N, Cs, Hs, Ws, Cb, ACT[c["act"]], stream())
    check(_from_layout(y, bl, N, Cb, H, W), _apply(r["convT_pre", null != "b"], c["act"]), what=tag + " convT fwd")
    dx = out(N * Cs * Hs * Ws, "small")
    call("dvae_convT4s2_dgrad", dy_big.p, BL, w.p, P(mask_small), dx.p, SL, N, Cs, Hs, Ws, Cb, stream())
    mult = 1.0 if null == "mask" else (r["mask_small"] > 0).double()
    check(_from_layout(dx, sl, N, Cs, Hs, Ws), r["convT_dx"] * mult, what=tag + " convT dgrad")
    dw, db = out(Cs * Cb * 16, "dw"), (None if null == "db" else out(Cb, "db"))
    call("dvae_convT4s2_wgrad", small.p, SL, dy_big.p, BL, dw.p, P(db), N, Cs, Hs, Ws, Cb, wsp, stream())
    check(dw.view.view(Cs, Cb, 4, 4), r["convT_dw"], what=tag + " convT wgrad")
    if db is not None:
        check(db.view, r["convT_db"], what=tag + " convT bias grad")
    for o in outs:
        assert o.guards_intact(), tag + ": a kernel wrote outside its output"


_CONV_ROLES = ("big", "small", "w", "b", "mask", "dw", "db", "ws")


def _conv_cases():
    c, t = KV.conv_case, KV.thin_case
    cases = [c(), t(), t(Cb=1)]
    # around the 32 <-> 32 base
    cases += [c(H=32, W=16), c(H=16, W=32)]
    cases += [c(Cb=v) for v in (16, 2, 33)] + [c(Cs=v) for v in (16, 1, 33)]
    cases += [c(bl="NCHW"), c(sl="NCHW"), c(bl="NCHW", sl="NCHW")]
    cases += [c(H=h, W=h) for h in (2, 4, 12, 64)]
    cases += [c(H=8, W=8), c(H=8, W=8, sl="NCHW"), c(H=8, W=8, bl="NCHW"), c(H=16, W=16)]        # the 4x4 end (its NCHW exception), 8x8
    cases += [c(act=a) for a in ("none", "sigmoid", "leaky")]
    # around the thin base
    for cb in (1, 3):
        cases += [t(Cb=cb, bl="NHWC"), t(Cb=cb, sl="NCHW"), t(Cb=cb, H=64, W=32), t(Cb=cb, H=32, W=64), t(Cb=cb, Cs=16)]
    cases += [t(Cb=2), t(Cb=4), t(act="sigmoid"), t(act="leaky"), t(act="none")]
    # the bias gradient of the transposed form at H != W through both generic weight-gradient forms: 3 * 32 * 16 positions =
    # one chunk of 1024 (k_wgrad_generic + k_chansum), 4 * 32 * 16 = two (k_wgrad_generic_part / _fin)
    cases += [t(Cb=1, H=64, W=32, N=4), t(Cb=3, H=32, W=64, N=4)]
    # NULL for every optional pointer, every pointer off the 16-byte grid
    for base in (c, t):
        cases += [base(null=n) for n in ("b", "db", "mask", "ws")]
        cases += [base(off=(role, nb)) for role in _CONV_ROLES for nb in (4, 8)]
    cases += [t(Cb=1, off=("big", 4)), t(Cb=1, off=("small", 8))]
    cases += [r.base for r in KV.PREDICATES if r.family == "conv"] + [r.neighbour for r in KV.PREDICATES if r.family == "conv" and r.neighbour]
    seen, uniq = set(), []
    for d in cases:
        if KV.conv_id(d) not in seen:
            seen.add(KV.conv_id(d))
            uniq.append(d)
    return uniq


@pytest.mark.parametrize("case", _conv_cases(), ids=KV.conv_id)
def test_conv_family(case):
    """dvae_conv4s2_{fwd,dgrad,wgrad} and dvae_convT4s2_{fwd,dgrad,wgrad} at one geometry / layout pair / activation / pointer
    set vs F.conv2d / F.conv_transpose2d and their autograd gradients in fp64."""
    _run_conv_family(case)


# ---- the fused last decoder layer -------------------------------------------------------------------------------------------------
def _fused_cases():
    t = KV.thin_case
    cases = [t(), t(Cb=1), t(Cb=2), t(Cb=4), t(Cs=16), t(sl="NCHW"), t(H=64, W=32), t(H=32, W=64), t(Cb=1, H=32, W=32)]
    cases += [t(null="b")] + [t(off=(role, nb)) for role in ("small", "w", "b") for nb in (4, 8)]
    cases += [r.base for r in KV.PREDICATES if r.family == "fused"] + [r.neighbour for r in KV.PREDICATES if r.family == "fused" and r.neighbour]
    seen, uniq = set(), []
    for d in cases:
        if KV.conv_id(d) not in seen:
            seen.add(KV.conv_id(d))
            uniq.append(d)
    return uniq


def _fused_args(c, dist, off_t=0, off_r=0, off_g=0):
    N, Cb, Cs, H, W, sl = c["N"], c["Cb"], c["Cs"], c["H"], c["W"], c["sl"]
    r = _conv_ref(N, Cb, Cs, H, W)
    role, nbytes = c["off"] or (None, 0)
    off = lambda name: nbytes if role == name else 0
    x, w = _in(_to_layout(torch.relu(r["small"]), sl), off("small")), _in(r["w"], off("w"))
    b = None if c["null"] == "b" else _in(r["b_big"], off("b"))
    tgt_cpu = torch.rand(N, Cb, H, W, generator=torch.Generator().manual_seed(11))
    tgt = _in(tgt_cpu, off_t)
    coef = torch.zeros(_lib.NCOEF)
    coef[_lib.C_INV_B] = 1.0 / N
    recon, g, parts = Buf(N * Cb * H * W, off_r), Buf(N * Cb * H * W, off_g), Buf(_lib.REC_NPART)
    args = (x.p, LAYOUT[sl], w.p, None if b is None else b.p, tgt.p, recon.p, g.p, _lib.REC[dist], _in(coef).p, parts.p, N, Cs,
            H // 2, W // 2, Cb, stream())
    return r, tgt_cpu, recon, g, parts, args


@pytest.mark.parametrize("case", _fused_cases(), ids=KV.conv_id)
def test_fused_likelihood(case):
    """dvae_convT4s2_sigmoid_recon_fwd beside its fused geometry (C in {1, 3}, 32 input channels NHWC, 32x32 -> 64x64): the
    neighbours take the two-pass form (a convT forward of run_up, then k_recon_loss); reference: the oracle's
    reconstruction_loss on the fp64 reconstruction."""
    c = case
    N, Cb, H, W = c["N"], c["Cb"], c["H"], c["W"]
    dist = ("bernoulli", "gaussian", "laplace")[(Cb + H // 32) % 3]
    r, tgt, recon, g, parts, args = _fused_args(c, dist)
    call("dvae_convT4s2_sigmoid_recon_fwd", *args)
    bias = None if c["null"] == "b" else r["b_big"].double()
    lr = F.conv_transpose2d(torch.relu(r["small"]).double(), r["w"].double(), bias, stride=2, padding=1).requires_grad_(True)
    ref_recon = torch.sigmoid(lr)
    loss = O.reconstruction_loss(tgt.double(), ref_recon, dist)
    loss.backward()
    tag = KV.conv_id(c) + " " + dist
    check(recon.view.view(N, Cb, H, W), ref_recon, what=tag + " fused recon")
    check(parts.view.sum() / N, loss, rtol=2e-5, what=tag + " fused loss")
    check(g.view.view(N, Cb, H, W), lr.grad, rtol=2e-4, atol_rel=2e-5, what=tag + " fused dL/dlogit")
    assert recon.guards_intact() and g.guards_intact() and parts.guards_intact()


@pytest.mark.parametrize("which", ["target", "recon", "g"])
@pytest.mark.parametrize("nbytes", [4, 8])
def test_fused_likelihood_refuses_an_unaligned_target_recon_or_gradient(which, nbytes):
    """Both forms of the entry point move target, recon and g in 16-byte accesses (the fused kernel, and k_recon_loss behind
    the two-pass form), so the entry refuses them off the 16-byte grid on the host, before any launch."""
    offs = {"off_t": 0, "off_r": 0, "off_g": 0}
    offs[{"target": "off_t", "recon": "off_r", "g": "off_g"}[which]] = nbytes
    r, tgt, recon, g, parts, args = _fused_args(KV.thin_case(), "bernoulli", **offs)
    with pytest.raises(DvaeHipError):
        call("dvae_convT4s2_sigmoid_recon_fwd", *args)
    assert _lib.lib().dvae_last_error()
    torch.cuda.synchronize()
    assert recon.untouched() and g.untouched() and parts.untouched()


# ---- refused arguments ------------------------------------------------------------------------------------------------------------
_BAD = [("Cin", 0), ("Cout", 0), ("H", 0), ("W", 0), ("H", 31), ("x_layout", 7), ("other_layout", 7)]
_REFUSED = [(e, n, v) for e in ("dvae_conv4s2_wgrad", "dvae_convT4s2_wgrad", "dvae_conv4s2_dgrad") for n, v in _BAD
            if not (e == "dvae_convT4s2_wgrad" and v == 31)]        # (H is the small side there: every positive height is a shape)


@pytest.mark.parametrize("entry,name,value", _REFUSED, ids=["%s-%s=%d" % r for r in _REFUSED])
def test_refused_arguments(entry, name, value):
    """The weight-gradient entries and the Conv2d input gradient refuse what their forward counterparts refuse -- an empty
    channel count or image, an odd height for the Conv2d forms, a layout code outside {NCHW, NHWC} -- on the host: DvaeHipError,
    a message in dvae_last_error, no output written."""
    a = dict(N=2, Cin=32, Cout=32, H=32, W=32, x_layout=_lib.NHWC, other_layout=_lib.NHWC)
    a[name] = value
    n = 2 * 32 * 64 * 64
    src1, src2, src3 = Buf(n), Buf(n), Buf(n)
    o1, o2 = Buf(n), Buf(64)
    ws = _ws()
    if entry == "dvae_conv4s2_dgrad":
        args = (src1.p, a["x_layout"], src2.p, src3.p, o1.p, a["other_layout"], a["N"], a["Cin"], a["H"], a["W"], a["Cout"], stream())
    else:
        args = (src1.p, a["x_layout"], src2.p, a["other_layout"], o1.p, o2.p, a["N"], a["Cin"], a["H"], a["W"], a["Cout"], ws, stream())
    with pytest.raises(DvaeHipError):
        call(entry, *args)
    assert _lib.lib().dvae_last_error()
    torch.cuda.synchronize()
    assert o1.untouched() and o2.untouched()


# ---- dvae_relayout ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,C,H,W", [(3, 1, 6, 6), (2, 3, 4, 10), (2, 3, 10, 4), (1, 32, 4, 4), (1, 5, 3, 7)])
def test_relayout_off_the_model_shape(N, C, H, W):
    """k_relayout at one channel, at H != W (both orders) and at one image, both directions, bit for bit against permute."""
    x = _rand(N, C, H, W, seed=1)
    a, out = _in(x.permute(0, 2, 3, 1)), Buf(x.numel())
    call("dvae_relayout", a.p, _lib.NHWC, out.p, N, C, H, W, stream())
    assert torch.equal(out.view.cpu().view(N, C, H, W), x) and out.guards_intact()
    back = Buf(x.numel())
    call("dvae_relayout", out.p, _lib.NCHW, back.p, N, C, H, W, stream())
    assert torch.equal(back.view.cpu().view(N, H, W, C), x.permute(0, 2, 3, 1)) and back.guards_intact()


# ---- the linear family ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lin_ref(M, K, N):
    r = dict(x=_rand(M, K, seed=1), w=_rand(N, K, seed=2, scale=1 / math.sqrt(K)), b=_rand(N, seed=3, scale=0.1),
             dy=_rand(M, N, seed=4), x_act=_rand(M, K, seed=5))
    x, w, b = (r[k].double().requires_grad_(True) for k in ("x", "w", "b"))
    pre = F.linear(x, w, b)
    pre.backward(r["dy"].double())
    r.update(pre=pre.detach(), dx=x.grad, dw=w.grad, db=b.grad)
    return r


_LIN_ROLES = ("x", "w", "b", "y", "dy", "x_act", "dx", "dw", "db")
# inside the acceptance region of: try_fc32<false> / <true> and try_fcw32 (8, 512, 256), (8, 256, 20); k_fc32's scalar-staging
# forms (8, 10, 256); try_gdma in both orientations and try_gdma_wgrad (64, 1000, 1000); try_narrow_* (100, 1000, 2);
# use_small (8, 1000, 36)
_LIN_BASES = [(8, 512, 256), (8, 256, 20), (8, 10, 256), (64, 1000, 1000), (100, 1000, 2), (8, 1000, 36)]


def _lin_cases():
    L = KV.lin_case
    cases = [L(M=m, K=k, N=n) for m, k, n in _LIN_BASES]
    # K % 4 (510, 1001), N % 4 (255, 18), the contraction past k_fc32's 512 in either direction (K = 516 | N = 516), ...
    cases += [L(K=510), L(M=64, K=1001, N=1000), L(N=255), L(K=256, N=18), L(K=516), L(N=516), L(M=64, K=1000, N=1001), L(M=64, K=1000, N=1002),
              L(M=8, K=1001, N=36), L(M=100, K=1001, N=2), L(M=130, K=512, N=256), L(M=63, K=1000, N=1000)]
    cases += [L(act="none"), L(act="leaky"), L(M=64, K=1000, N=1000, act="leaky")]
    for m, k, n in _LIN_BASES:
        cases += [L(M=m, K=k, N=n, off=(role, nb)) for role in _LIN_ROLES for nb in (4, 8)]
    cases += [r.base for r in KV.PREDICATES if r.family == "linear"] + [r.neighbour for r in KV.PREDICATES if r.family == "linear" and r.neighbour]
    seen, uniq = set(), []
    for d in cases:
        if KV.lin_id(d) not in seen:
            seen.add(KV.lin_id(d))
            uniq.append(d)
    return uniq


@pytest.mark.parametrize("case", _lin_cases(), ids=KV.lin_id)
def test_linear_family(case):
    """dvae_linear_fwd, dvae_linear_dgrad (no mask, ReLU mask, LeakyReLU mask) and dvae_linear_wgrad, each without and with the
    workspace, vs F.linear and its autograd gradients in fp64."""
    M, K, N, act = case["M"], case["K"], case["N"], case["act"]
    r = _lin_ref(M, K, N)
    role, nbytes = case["off"] or (None, 0)
    off = lambda name: nbytes if role == name else 0
    tag = KV.lin_id(case)
    x, w, b, dy, x_act = (_in(r[k], off(k)) for k in ("x", "w", "b", "dy", "x_act"))
    outs = []

    def out(n, name):
        o = Buf(n, off(name))
        outs.append(o)
        return o

    for wsp in (None, _ws()):
        sp = " (ws)" if wsp else ""
        y = out(M * N, "y")
        call("dvae_linear_fwd", x.p, w.p, b.p, y.p, M, K, N, ACT[act], wsp, stream())
        check(y.view.view(M, N), _apply(r["pre"], act), what=tag + " linear fwd" + sp)
        dw, db = out(N * K, "dw"), out(N, "db")
        call("dvae_linear_wgrad", x.p, dy.p, dw.p, db.p, M, K, N, wsp, stream())
        check(dw.view.view(N, K), r["dw"], what=tag + " linear wgrad" + sp)
        check(db.view, r["db"], what=tag + " linear bias grad" + sp)
        for mact in ("none", "relu", "leaky"):
            mult = {"none": torch.ones_like(r["x_act"]), "relu": (r["x_act"] > 0).float(),
                    "leaky": torch.where(r["x_act"] > 0, 1.0, 0.2)}[mact]
            dx = out(M * K, "dx")
            call("dvae_linear_dgrad", dy.p, w.p, None if mact == "none" else x_act.p, ACT[mact], dx.p, M, K, N, wsp, stream())
            check(dx.view.view(M, K), r["dx"] * mult.double(), what=tag + " linear dgrad mask=" + mact + sp)
    for o in outs:
        assert o.guards_intact(), tag + ": a kernel wrote outside its output"


def test_linear_null_bias_and_bias_gradient():
    """b == NULL on the forward and db == NULL on the weight gradient, on each forward / weight-gradient kernel family."""
    for M, K, N in _LIN_BASES + [(8, 510, 256)]:
        r = _lin_ref(M, K, N)
        x, w, dy = _in(r["x"]), _in(r["w"]), _in(r["dy"])
        y, dw = Buf(M * N), Buf(N * K)
        call("dvae_linear_fwd", x.p, w.p, None, y.p, M, K, N, _lib.ACT_NONE, None, stream())
        check(y.view.view(M, N), r["pre"] - r["b"].double(), what="linear fwd b=NULL %s" % ((M, K, N),))
        call("dvae_linear_wgrad", x.p, dy.p, dw.p, None, M, K, N, None, stream())
        check(dw.view.view(N, K), r["dw"], what="linear wgrad db=NULL %s" % ((M, K, N),))
        assert y.guards_intact() and dw.guards_intact()


# (K, N, byte offset of x, of dy) -> flags bit 1 (16-byte loads of x: K % 4 == 0 and x aligned), bit 0 (of dy: N % 4 == 0, aligned)
_GROUPED = [(512, 256, 0, 0), (256, 18, 0, 0), (10, 256, 0, 0), (256, 20, 0, 4), (256, 20, 8, 0), (7, 33, 4, 8)]


@pytest.mark.parametrize("M", [8, 130])
def test_linear_wgrad_grouped_flag_bits(M):
    """launch_linear_wgrad_grouped's two per-problem flags (linear_grouped.hip:161), each at 0 and at 1, and each cleared by
    either of its two terms: the row length and the base pointer."""
    probs, refs, outs = [], [], []
    for q, (K, N, ox, ody) in enumerate(_GROUPED):
        x, dy = _rand(M, K, seed=10 + q), _rand(M, N, seed=30 + q)
        dw, db = Buf(N * K), Buf(N)
        probs.append((_in(x, ox).p, _in(dy, ody).p, dw.p, db.p, M, K, N))
        refs.append((dy.double().t() @ x.double(), dy.double().sum(0)))
        outs.append((dw, db, N, K))
    arr, addr = _lib.wgrad_descs(probs)
    call("dvae_linear_wgrad_grouped", addr, len(probs), stream())
    for q, ((dw, db, N, K), (rw, rb)) in enumerate(zip(outs, refs)):
        check(dw.view.view(N, K), rw, what="grouped wgrad dw[%d] M=%d" % (q, M))
        check(db.view, rb, what="grouped wgrad db[%d] M=%d" % (q, M))
        assert dw.guards_intact() and db.guards_intact()
