"""-m gpu: the memory contract of every launching entry point of include/dvae_hip.h, on guard-banded, poisoned buffers
(tests/guard_util.py).

For one call of an entry point the contract is: nothing is written outside the arguments' documented sizes (front and back
guards keep their poison), inputs come back bit-identical, every output element the header defines is written, and the
outputs are finite and bit-identical whether the call runs on ordinary tensors, on NaN-poisoned 256-byte aligned buffers (A)
or on buffers at the weakest documented alignment whose surroundings hold -1e30 (B).  Bit-identity with the plain run ties
these runs to the values the parity tests check, so this file carries no references of its own.

Masked as "documented unused" (every mask cites the header): rowstats columns >= 4 + D, the slots of `scal` that the DVAE_S_*
enum does not name, kl_dim[D, 16) and -- for dvae_reparam_kl_fwd without coef -- kl_dim[0, 16).  Nothing else.

Alignment in variant B is 16 bytes (the parameter arena's granularity) except where the header promises less: uint8 targets of
dvae_recon_rows (4), `out` of dvae_image_grid_u8 (any), every tensor of dvae_linear_wgrad_grouped (4: "rows need no alignment").

Wall time on one MI355X, one pytest process each (measured): this file + tests/test_gpu_step_poison.py 10 s (669 tests; pytest
reports 7.7 s); the rest of `pytest tests -m gpu` 223 s (418 passed, 19 skipped for want of more GPUs; pytest reports 221 s).

First run on a device: every spec passed -- no kernel wrote outside its arguments, left a defined element unwritten or let its
result depend on memory it does not own; both device sensitivity checks raised as they must.
"""
import ctypes
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import force_generic, stream
from disvae_amd import _lib
from guard_util import run_contract, GuardError
from test_gpu_fused_core import _conv_image, _fc_images, _thin_records, _fc_params

# seconds on one MI355X, one pytest process each: (this file + tests/test_gpu_step_poison.py, the rest of `pytest tests -m gpu`)
WALL_TIME = (10, 223)

NCHW, NHWC = _lib.NCHW, _lib.NHWC
RELU, NONE, SIG, LEAKY = _lib.ACT_RELU, _lib.ACT_NONE, _lib.ACT_SIGMOID, _lib.ACT_LEAKY02
F32, U8, I32, I64 = torch.float32, torch.uint8, torch.int32, torch.int64


class Spec:
    def __init__(self, id, entry, build, generic=False):
        self.id, self.entry, self.build, self.generic = id, entry, build, generic


SPECS = []


def spec(id, entry, generic=False):
    def deco(build):
        SPECS.append(Spec(id, entry, build, generic))
        return build
    return deco


@functools.lru_cache(maxsize=64)
def R(shape, seed=0, scale=1.0):
    """Seeded uniform [-scale, scale) CPU tensor (cached: the three runs of a spec get the same data)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def P(shape, seed=0):
    """post-ReLU activation"""
    return torch.relu(R(shape, seed))


def U(shape, seed=0):
    return (R(shape, seed) + 1) * 0.5


@functools.lru_cache(maxsize=16)
def BYTES(shape, seed=0):
    return torch.randint(0, 256, shape, dtype=U8, generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=16)
def BITS(n, seed=0):
    return torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), dtype=torch.int64, generator=torch.Generator().manual_seed(seed)).to(I32)


@functools.lru_cache(maxsize=4)
def THIN(C):
    """(weight, its staged pair records) of the last decoder layer"""
    w = R((32, C, 4, 4), 2, 0.2)
    return w, _thin_records(w)


def coef_vec(inv_b=0.125):
    c = torch.zeros(_lib.NCOEF)
    c[_lib.C_INV_B], c[_lib.C_ANNEAL], c[_lib.C_BETA] = inv_b, 0.3, 4.0
    c[_lib.C_ALPHA], c[_lib.C_GAMMA], c[_lib.C_CAP] = 1.0, 2.0, 7.0
    return c


def ws_floats():
    return int(_lib.lib().dvae_conv_wgrad_ws_floats())


def act(N, C, H, layout):
    return (N, H, H, C) if layout == NHWC else (N, C, H, H)


def ptr(g):
    return None if g is None else g.ptr


# ===== conv ends and stack ======================================================================================================
# (N, C) at the 64x64 thin ends: smallest, below a tile, straddling tiles (33, 70), and the batches where the wave-specialised
# kernels of conv_thin_ws.hip take over (193, 200)
THIN64 = [(1, 1), (1, 3), (3, 1), (3, 3), (33, 3), (70, 1), (193, 1), (200, 3)]
THIN32 = [(1, 1), (3, 3), (33, 1), (70, 3)]                       # 32x32 images (k_down_thin_px / k_up_thin_px)
TUNED = [1, 3, 33, 70]
# (N, Cb = channels of the big side, Hb = its height, layout of the small side, generic)
GEOM = ([(N, C, 64, NHWC, False) for N, C in THIN64] + [(N, C, 32, NHWC, False) for N, C in THIN32] +
        [(N, 32, Hb, NHWC, False) for Hb in (32, 16, 8) for N in TUNED] + [(N, 32, 8, NCHW, False) for N in TUNED] +
        [(1, 3, 64, NHWC, True), (5, 1, 64, NHWC, True), (5, 1, 32, NHWC, True), (5, 32, 16, NHWC, True), (1, 32, 8, NCHW, True),
         (5, 32, 32, NHWC, True)])


def _gid(N, Cb, Hb, sl, generic):
    return "N%d-C%d-H%d-%s%s" % (N, Cb, Hb, "nhwc" if sl == NHWC else "nchw", "-generic" if generic else "")


def _conv_specs():
    for k, (N, Cb, Hb, sl, generic) in enumerate(GEOM):
        gid = _gid(N, Cb, Hb, sl, generic)
        bl = NHWC if Cb == 32 else NCHW           # the thin side is the API boundary: NCHW
        Hs = Hb // 2
        big, small = act(N, Cb, Hb, bl), act(N, 32, Hs, sl)

        # Conv2d: big -> small, w[32][Cb][4][4]
        def conv_fwd(al, N=N, Cb=Cb, Hb=Hb, bl=bl, sl=sl, big=big, small=small):
            x, w, b = al.inp("x", R(big, 1)), al.inp("w", R((32, Cb, 4, 4), 2, 0.2)), al.inp("b", R((32,), 3, 0.1))
            return [x, bl, w, b, al.out("y", small), sl, N, Cb, Hb, Hb, 32, RELU, stream()]
        SPECS.append(Spec("conv4s2_fwd-" + gid, "dvae_conv4s2_fwd", conv_fwd, generic))

        def conv_wgrad(al, N=N, Cb=Cb, Hb=Hb, bl=bl, sl=sl, big=big, small=small, no_db=(k == 2)):
            x, dy = al.inp("x", R(big, 1)), al.inp("dy", R(small, 4))
            dw = al.out("dw", (32, Cb, 4, 4))
            db = None if no_db else al.out("db", (32,))
            return [x, bl, dy, sl, dw, db, N, Cb, Hb, Hb, 32, al.ws("ws", (ws_floats(),)), stream()]
        SPECS.append(Spec("conv4s2_wgrad-" + gid, "dvae_conv4s2_wgrad", conv_wgrad, generic))

        if Cb == 32:
            def conv_dgrad(al, N=N, Cb=Cb, Hb=Hb, bl=bl, sl=sl, big=big, small=small):
                dy, w, xa = al.inp("dy", R(small, 4)), al.inp("w", R((32, Cb, 4, 4), 2, 0.2)), al.inp("x_act", P(big, 5))
                return [dy, sl, w, xa, al.out("dx", big), bl, N, Cb, Hb, Hb, 32, stream()]
            SPECS.append(Spec("conv4s2_dgrad-" + gid, "dvae_conv4s2_dgrad", conv_dgrad, generic))

        # ConvTranspose2d: small -> big, w[32][Cb][4][4]
        def convT_fwd(al, N=N, Cb=Cb, Hs=Hs, bl=bl, sl=sl, big=big, small=small):
            x, w, b = al.inp("x", P(small, 1)), al.inp("w", R((32, Cb, 4, 4), 2, 0.2)), al.inp("b", R((Cb,), 3, 0.1))
            return [x, sl, w, b, al.out("y", big), bl, N, 32, Hs, Hs, Cb, RELU if Cb == 32 else SIG, stream()]
        SPECS.append(Spec("convT4s2_fwd-" + gid, "dvae_convT4s2_fwd", convT_fwd, generic))

        def convT_dgrad(al, N=N, Cb=Cb, Hs=Hs, bl=bl, sl=sl, big=big, small=small):
            dy, w, xa = al.inp("dy", R(big, 4)), al.inp("w", R((32, Cb, 4, 4), 2, 0.2)), al.inp("x_act", P(small, 1))
            return [dy, bl, w, xa, al.out("dx", small), sl, N, 32, Hs, Hs, Cb, stream()]
        SPECS.append(Spec("convT4s2_dgrad-" + gid, "dvae_convT4s2_dgrad", convT_dgrad, generic))

        def convT_wgrad(al, N=N, Cb=Cb, Hs=Hs, bl=bl, sl=sl, big=big, small=small, no_db=(k == 3)):
            x, dy = al.inp("x", P(small, 1)), al.inp("dy", R(big, 4))
            dw = al.out("dw", (32, Cb, 4, 4))
            db = None if no_db else al.out("db", (Cb,))
            return [x, sl, dy, bl, dw, db, N, 32, Hs, Hs, Cb, al.ws("ws", (ws_floats(),)), stream()]
        SPECS.append(Spec("convT4s2_wgrad-" + gid, "dvae_convT4s2_wgrad", convT_wgrad, generic))

        if Cb != 32:
            def recon(al, N=N, Cb=Cb, Hs=Hs, Hb=Hb, dist=k % 3):
                x, w, b = al.inp("x", P((N, Hs, Hs, 32), 1)), al.inp("w", R((32, Cb, 4, 4), 2, 0.2)), al.inp("b", R((Cb,), 3, 0.1))
                t, c = al.inp("target", U((N, Cb, Hb, Hb), 6)), al.inp("coef", coef_vec(1.0 / N))
                return [x, NHWC, w, b, t, al.out("recon", (N, Cb, Hb, Hb)), al.out("g", (N, Cb, Hb, Hb)), dist, c,
                        al.out("partials", (_lib.REC_NPART,)), N, 32, Hs, Hs, Cb, stream()]
            SPECS.append(Spec("convT4s2_sigmoid_recon_fwd-" + gid, "dvae_convT4s2_sigmoid_recon_fwd", recon, generic))


_conv_specs()


# ---- uint8 forms, bit planes, staged weights (64x64 geometry only) ---------------------------------------------------------------
def _u8_specs():
    for N, C in THIN64:
        gid = "N%d-C%d" % (N, C)

        def fwd_u8(al, N=N, C=C):
            x, w, b = al.inp("x", BYTES((N, C, 64, 64), 1)), al.inp("w", R((32, C, 4, 4), 2, 0.2)), al.inp("b", R((32,), 3, 0.1))
            return [x, w, b, al.out("y", (N, 32, 32, 32)), N, C, 64, 64, 32, RELU, stream()]
        SPECS.append(Spec("conv4s2_fwd_u8-" + gid, "dvae_conv4s2_fwd_u8", fwd_u8))

        def wgrad_u8(al, N=N, C=C, no_db=(N == 3 and C == 1)):
            x, dy = al.inp("x", BYTES((N, C, 64, 64), 1)), al.inp("dy", R((N, 32, 32, 32), 4))
            db = None if no_db else al.out("db", (32,))
            return [x, dy, al.out("dw", (32, C, 4, 4)), db, N, C, 64, 64, 32, al.ws("ws", (ws_floats(),)), stream()]
        SPECS.append(Spec("conv4s2_wgrad_u8-" + gid, "dvae_conv4s2_wgrad_u8", wgrad_u8))

        def recon_u8(al, N=N, C=C, dist=(N + C) % 3):
            x, w, b = al.inp("x", P((N, 32, 32, 32), 1)), al.inp("w", R((32, C, 4, 4), 2, 0.2)), al.inp("b", R((C,), 3, 0.1))
            t, c = al.inp("target", BYTES((N, C, 64, 64), 6)), al.inp("coef", coef_vec(1.0 / N))
            return [x, w, b, t, al.out("recon", (N, C, 64, 64)), al.out("g", (N, C, 64, 64)), dist, c,
                    al.out("partials", (_lib.REC_NPART,)), N, 32, 32, 32, C, stream()]
        SPECS.append(Spec("convT4s2_sigmoid_recon_fwd_u8-" + gid, "dvae_convT4s2_sigmoid_recon_fwd_u8", recon_u8))

        for u8 in (0, 1):
            def conv1_bits(al, N=N, C=C, u8=u8):
                x = al.inp("x", BYTES((N, C, 64, 64), 1) if u8 else U((N, C, 64, 64), 1))
                w, b = al.inp("w", R((32, C, 4, 4), 2, 0.2)), al.inp("b", R((32,), 3, 0.1))
                return [x, u8, w, b, al.out("y", (N, 32, 32, 32)), al.out("y_bits", (N * 1024,), dtype=I32), N, C, stream()]
            SPECS.append(Spec("conv1_fwd_bits-%s-%s" % (gid, "u8" if u8 else "f32"), "dvae_conv1_fwd_bits", conv1_bits))

        def dgrad_bits(al, N=N, C=C):
            dy, w, bits = al.inp("dy", R((N, C, 64, 64), 4)), al.inp("w", R((32, C, 4, 4), 2, 0.2)), al.inp("x_act_bits", BITS(N * 1024, 7))
            return [dy, w, bits, al.out("dx", (N, 32, 32, 32)), N, C, stream()]
        SPECS.append(Spec("convT3_dgrad_bits-" + gid, "dvae_convT3_dgrad_bits", dgrad_bits))

        for tgt in ("none", "f32", "u8"):
            def staged(al, N=N, C=C, tgt=tgt, dist=(N + C) % 3):
                x, img, b = al.inp("x", P((N, 32, 32, 32), 1)), al.inp("img_pairs", THIN(C)[1]), al.inp("b", R((C,), 3, 0.1))
                recon = al.out("recon", (N, C, 64, 64))
                if tgt == "none":
                    return [x, img, b, None, 0, recon, None, 0, None, None, N, C, stream()]
                t = al.inp("target", BYTES((N, C, 64, 64), 6) if tgt == "u8" else U((N, C, 64, 64), 6))
                c = al.inp("coef", coef_vec(1.0 / N))
                return [x, img, b, t, int(tgt == "u8"), recon, al.out("g", (N, C, 64, 64)), dist, c,
                        al.out("partials", (_lib.REC_NPART,)), N, C, stream()]
            SPECS.append(Spec("convT3_fwd_staged-%s-%s" % (gid, tgt), "dvae_convT3_fwd_staged", staged))


_u8_specs()


def _staged32_specs():
    w = R((32, 32, 4, 4), 2, 0.2)
    for Hs in (16, 8, 4):
        for N in TUNED + ([200] if Hs == 16 else []):
            for lay in [NHWC] + ([NCHW] if Hs == 4 else []):
                gid = "N%d-Hs%d-%s" % (N, Hs, "nhwc" if lay == NHWC else "nchw")
                big, small = (N, 2 * Hs, 2 * Hs, 32), act(N, 32, Hs, lay)
                for form in ("fwd", "dgrad"):
                    def down(al, N=N, Hs=Hs, lay=lay, big=big, small=small, form=form):
                        x, img = al.inp("big", R(big, 1)), al.inp("img_down", _conv_image(w, True))
                        bias = al.inp("bias", R((32,), 3, 0.1)) if form == "fwd" else None
                        mask = al.inp("mask", P(small, 5)) if form == "dgrad" else None
                        return [x, img, bias, mask, al.out("out", small), lay, N, Hs, RELU if form == "fwd" else NONE, stream()]
                    SPECS.append(Spec("conv32_down-%s-%s" % (gid, form), "dvae_conv32_down", down))

                    def up(al, N=N, Hs=Hs, lay=lay, big=big, small=small, form=form):
                        x, img = al.inp("small", P(small, 5)), al.inp("img_up", _conv_image(w, False))
                        bias = al.inp("bias", R((32,), 3, 0.1)) if form == "fwd" else None
                        mask = al.inp("mask", P(big, 7)) if form == "dgrad" else None
                        return [x, lay, img, bias, mask, al.out("out", big), N, Hs, RELU if form == "fwd" else NONE, stream()]
                    SPECS.append(Spec("conv32_up-%s-%s" % (gid, form), "dvae_conv32_up", up))
    for N in TUNED + [200]:
        for form in ("fwd", "dgrad"):
            def up_bits(al, N=N, form=form):
                x, img = al.inp("small", P((N, 16, 16, 32), 5)), al.inp("img_up", _conv_image(w, False))
                if form == "fwd":
                    return [x, img, al.inp("bias", R((32,), 3, 0.1)), None, al.out("out", (N, 32, 32, 32)),
                            al.out("out_bits", (N * 1024,), dtype=I32), N, RELU, stream()]
                return [x, img, None, al.inp("mask_bits", BITS(N * 1024, 7)), al.out("out", (N, 32, 32, 32)), None, N, NONE, stream()]
            SPECS.append(Spec("conv32_up_bits-N%d-%s" % (N, form), "dvae_conv32_up_bits", up_bits))


_staged32_specs()


@spec("stage_weights-all", "dvae_stage_weights")
def _stage_all(al):
    shapes = [(256, 512), (20, 256), (256, 10), (512, 256), (2, 256), (256, 1)]
    cd = al.keep((_lib.ConvImageDesc * 2)())
    for q, d in enumerate(cd):
        d.w = al.inp("conv_w%d" % q, R((32, 32, 4, 4), 10 + q)).ptr
        d.img_down = al.out("img_down%d" % q, (16384,)).ptr
        d.img_up = al.out("img_up%d" % q, (16384,)).ptr if q == 0 else None
    fd = al.keep((_lib.FcImageDesc * len(shapes))())
    for q, (d, (N, K)) in enumerate(zip(fd, shapes)):
        d.w = al.inp("fc_w%d" % q, R((N, K), 20 + q)).ptr
        d.img_fwd = al.out("img_fwd%d" % q, ((K + 3) // 4 * N * 4,)).ptr
        d.img_bwd = al.out("img_bwd%d" % q, ((N + 3) // 4 * K * 4,)).ptr
        d.N, d.K = N, K
    td = al.keep(_lib.ThinImageDesc())
    td.w, td.img_pairs, td.C = al.inp("thin_w", R((32, 3, 4, 4), 30)).ptr, al.out("img_pairs", (32 * _lib.thin_pair_floats(3),)).ptr, 3
    cv = al.keep((ctypes.c_float * 8)(0.5, 1.5, 2.5, 3.5, 4.5, 5.5, 6.5, 7.5))
    return [ctypes.addressof(cd), 2, ctypes.addressof(fd), len(shapes), ctypes.addressof(td), al.out("coef", (8,)), ctypes.addressof(cv),
            stream()]


@spec("stage_weights-thin1-coef", "dvae_stage_weights")
def _stage_thin1(al):
    td = al.keep(_lib.ThinImageDesc())
    td.w, td.img_pairs, td.C = al.inp("thin_w", R((32, 1, 4, 4), 30)).ptr, al.out("img_pairs", (32 * _lib.thin_pair_floats(1),)).ptr, 1
    cv = al.keep((ctypes.c_float * 8)(*[1.0] * 8))
    return [None, 0, None, 0, ctypes.addressof(td), al.out("coef", (8,)), ctypes.addressof(cv), stream()]


# ===== linear ===================================================================================================================
LINEAR = [(1, 256, 512), (7, 10, 256), (33, 256, 20), (100, 1000, 2), (130, 16, 600), (200, 300, 260), (1030, 1000, 1000)]


def _linear_specs():
    for q, (M, K, N) in enumerate(LINEAR):
        for use_ws in (False, True):
            gid = "M%d-K%d-N%d-%s" % (M, K, N, "ws" if use_ws else "nows")
            a = (RELU, NONE, LEAKY)[q % 3]

            def fwd(al, M=M, K=K, N=N, use_ws=use_ws, a=a):
                x, w, b = al.inp("x", R((M, K), 1)), al.inp("w", R((N, K), 2, 1 / math.sqrt(K))), al.inp("b", R((N,), 3, 0.1))
                y = al.out("y", (M, N))
                return [x, w, b, y, M, K, N, a, al.ws("ws", (ws_floats(),)) if use_ws else None, stream()]
            SPECS.append(Spec("linear_fwd-" + gid, "dvae_linear_fwd", fwd))

            def dgrad(al, M=M, K=K, N=N, use_ws=use_ws, a=a, q=q):
                dy, w = al.inp("dy", R((M, N), 4)), al.inp("w", R((N, K), 2, 1 / math.sqrt(K)))
                xa = al.inp("x_act", R((M, K), 5)) if a != NONE else None
                dx = al.out("dx", (M, K))
                return [dy, w, xa, a, dx, M, K, N, al.ws("ws", (ws_floats(),)) if use_ws else None, stream()]
            SPECS.append(Spec("linear_dgrad-" + gid, "dvae_linear_dgrad", dgrad))

            def wgrad(al, M=M, K=K, N=N, use_ws=use_ws, no_db=(q == 1)):
                x, dy = al.inp("x", R((M, K), 1)), al.inp("dy", R((M, N), 4))
                dw = al.out("dw", (N, K))
                db = None if no_db else al.out("db", (N,))
                return [x, dy, dw, db, M, K, N, al.ws("ws", (ws_floats(),)) if use_ws else None, stream()]
            SPECS.append(Spec("linear_wgrad-" + gid, "dvae_linear_wgrad", wgrad))
    shapes = [(512, 256), (256, 512), (256, 256), (10, 256), (256, 20), (7, 33), (100, 36), (256, 256)]   # (K, N)
    for M in (3, 100, 1500):
        def grouped(al, M=M):
            probs = []
            for q, (K, N) in enumerate(shapes):
                # include/dvae_hip.h, dvae_linear_wgrad_grouped: "rows need no alignment" -> the natural 4 bytes of a float
                x, dy = al.inp("x%d" % q, R((M, K), 10 + q), align=4), al.inp("dy%d" % q, R((M, N), 30 + q), align=4)
                dw = al.out("dw%d" % q, (N, K), align=4)
                db = None if q == 5 else al.out("db%d" % q, (N,), align=4)
                probs.append((x.ptr, dy.ptr, dw.ptr, ptr(db), M, K, N))
            arr, addr = _lib.wgrad_descs(probs)
            al.keep(arr)
            return [addr, len(probs), stream()]
        SPECS.append(Spec("linear_wgrad_grouped-M%d" % M, "dvae_linear_wgrad_grouped", grouped))


_linear_specs()


# ===== FC chain =================================================================================================================
@functools.lru_cache(maxsize=8)
def _fc(D):
    shapes, W, Bv = _fc_params(D, seed=3)
    return shapes, {k: _fc_images(W[k]) for k in shapes}, Bv


_WC, _WT = R((32, 32, 4, 4), 31, 0.2), R((32, 32, 4, 4), 32, 0.2)


def _chain_fwd(n_enc, n_kl, n_dec, D, noise=True, ends=False):
    def build(al):
        shapes, img, Bv = _fc(D)
        f = {}
        for k in shapes:
            f["w_" + k] = al.inp("w_" + k, img[k][0]).ptr
            f["b_" + k] = al.inp("b_" + k, Bv[k]).ptr
        if noise:
            f["eps"] = al.inp("eps", R((n_enc, D), 2)).ptr
        if ends:
            f["conv_in"] = al.inp("conv_in", P((n_enc, 8, 8, 32), 41)).ptr
            f["conv_w"] = al.inp("conv_w", _conv_image(_WC, True)).ptr
            f["conv_b"] = al.inp("conv_b", R((32,), 33, 0.1)).ptr
            f["a_flat"] = al.out("a_flat", (n_enc, 512)).ptr          # an OUTPUT of the launch when conv_in is given
            if n_dec:
                f["convT_w"] = al.inp("convT_w", _conv_image(_WT, False)).ptr
                f["convT_b"] = al.inp("convT_b", R((32,), 34, 0.1)).ptr
                f["convT_out"] = al.out("convT_out", (n_dec, 8, 8, 32)).ptr
        else:
            f["a_flat"] = al.inp("a_flat", P((n_enc, 512), 1)).ptr
        for k, wd in (("h1", 256), ("h2", 256), ("ml", 2 * D), ("mu", D), ("logvar", D), ("z", D)):
            f[k] = al.out(k, (n_enc, wd)).ptr
        rows = _lib.fc_chain_rows(n_enc)
        f["kl_part"] = al.out("kl_part", ((n_enc + rows - 1) // rows, 16)).ptr
        if n_dec:
            for k, wd in (("d1", 256), ("d2", 256), ("d3", 512)):
                f[k] = al.out(k, (n_dec, wd)).ptr
        st, addr = _lib.struct_of(_lib.FcChainFwdArgs, n_enc=n_enc, n_kl=n_kl, n_dec=n_dec, D=D, **f)
        al.keep(st)
        return [addr, stream()]
    return build


def _chain_bwd(n, D, noise=True, extra=1, with_dz=True, ends=False):
    def build(al):
        shapes, img, Bv = _fc(D)
        f = {}
        for k in shapes:
            f["w_" + k] = al.inp("w_" + k, img[k][1]).ptr
        for i, (k, wd) in enumerate([("d2", 256), ("d1", 256), ("h2", 256), ("h1", 256), ("a_flat", 512)]):
            f[k] = al.inp(k, P((n, wd), 10 + i)).ptr
        f["mu"], f["logvar"] = al.inp("mu", R((n, D), 20)).ptr, al.inp("logvar", R((n, D), 21, 0.7)).ptr
        if noise:
            f["eps"] = al.inp("eps", R((n, D), 3)).ptr
        if extra:
            f["dz2"] = al.inp("dz2", R((n, D), 22)).ptr
        if extra == 2:
            f["dz3"] = al.inp("dz3", R((n, D), 23)).ptr
        if extra == 1:
            f["dmu_x"], f["dlv_x"] = al.inp("dmu_x", R((n, D), 24)).ptr, al.inp("dlv_x", R((n, D), 25)).ptr
        scal = torch.zeros(_lib.NSCAL)
        scal[_lib.S_KLW] = 1.7
        f["scal"], f["coef"] = al.inp("scal", scal).ptr, al.inp("coef", coef_vec(1.0 / n)).ptr
        if ends:
            f["convT_gout"] = al.inp("convT_gout", R((n, 8, 8, 32), 51)).ptr
            f["convT_w"] = al.inp("convT_w", _conv_image(_WT, True)).ptr
            f["d3"] = al.inp("d3", P((n, 512), 65)).ptr
            f["gd3"] = al.out("gd3", (n, 512)).ptr                     # an OUTPUT of the launch when convT_gout is given
            f["conv_w"] = al.inp("conv_w", _conv_image(_WC, False)).ptr
            f["conv_act"] = al.inp("conv_act", P((n, 8, 8, 32), 71)).ptr
            f["conv_gin"] = al.out("conv_gin", (n, 8, 8, 32)).ptr
        else:
            f["gd3"] = al.inp("gd3", R((n, 512), 1)).ptr
        for k, wd in (("gd2", 256), ("gd1", 256), ("dml", 2 * D), ("gh2", 256), ("gh1", 256), ("ga_flat", 512)):
            f[k] = al.out(k, (n, wd)).ptr
        if with_dz:
            f["dz"] = al.out("dz", (n, D)).ptr
        st, addr = _lib.struct_of(_lib.FcChainBwdArgs, n=n, D=D, **f)
        al.keep(st)
        return [addr, stream()]
    return build


def _chain_specs():
    for ends in (False, True):
        e = "-ends" if ends else ""
        for n, D in [(1, 10), (5, 10), (130, 10), (1027, 10), (5, 1), (130, 16), (1, 16), (1027, 1)]:
            SPECS.append(Spec("fc_chain_fwd-n%d-D%d%s" % (n, D, e), "dvae_fc_chain_fwd", _chain_fwd(n, n, n, D, ends=ends)))
            SPECS.append(Spec("fc_chain_bwd-n%d-D%d%s" % (n, D, e), "dvae_fc_chain_bwd",
                              _chain_bwd(n, D, extra=1 + (n % 2), ends=ends)))
        SPECS.append(Spec("fc_chain_fwd-factor-130-65%s" % e, "dvae_fc_chain_fwd", _chain_fwd(130, 65, 65, 10, ends=ends)))
        SPECS.append(Spec("fc_chain_fwd-n5-no-eps%s" % e, "dvae_fc_chain_fwd", _chain_fwd(5, 5, 5, 10, noise=False, ends=ends)))
        SPECS.append(Spec("fc_chain_fwd-n130-no-decoder%s" % e, "dvae_fc_chain_fwd", _chain_fwd(130, 130, 0, 10, ends=ends)))
        SPECS.append(Spec("fc_chain_bwd-n5-no-eps%s" % e, "dvae_fc_chain_bwd", _chain_bwd(5, 10, noise=False, extra=0, ends=ends)))
        SPECS.append(Spec("fc_chain_bwd-n130-no-dz%s" % e, "dvae_fc_chain_bwd", _chain_bwd(130, 10, with_dz=False, ends=ends)))


_chain_specs()


# ===== latent / loss ============================================================================================================
def _kl_blocks(B):
    return int(_lib.lib().dvae_reparam_kl_blocks(B))


def _reparam_fwd(B, D, form):
    """form: "coef" (final values), "blocks" (coef NULL: partial blocks only), "eval" (eps, kl_dim, coef NULL)."""
    def build(al):
        ml = al.inp("ml", R((B, 2 * D), 1, 1.5))
        eps = al.inp("eps", R((B, D), 2)) if form != "eval" else None
        mu, lv, z = al.out("mu", (B, D)), al.out("logvar", (B, D)), al.out("z", (B, D))
        kl, coef = None, None
        if form != "eval":
            if D > _lib.MAX_LATENT_DIM:
                kl = al.out("kl_dim", (D,))          # "above, kl_dim is just the D final values" (dvae_hip.h, dvae_reparam_kl_fwd)
            else:
                nb = _kl_blocks(B)
                m = torch.zeros(16 + nb * 16, dtype=torch.bool)
                m[16:] = True                        # "the rest (kl_dim + 16) holds per-workgroup partial sums, blocks of 16 floats"
                if form == "coef":
                    m[:D] = True                     # "[0,D) = coef[INV_B] * sum_b ..."; kl_dim[D, 16) is not defined by the header;
                kl = al.out("kl_dim", (16 + nb * 16,), written=m)     # coef == NULL: "only the ... partial blocks are written"
            if form == "coef":
                coef = al.inp("coef", coef_vec(1.0 / B))
        return [ml, eps, mu, lv, z, kl, coef, B, D, stream()]
    return build


def _latent_specs():
    for B in (1, 2, 200, 1500):
        for form in ("coef", "blocks", "eval"):
            SPECS.append(Spec("reparam_kl_fwd-B%d-D10-%s" % (B, form), "dvae_reparam_kl_fwd", _reparam_fwd(B, 10, form)))
    for B, D in ((5, 1), (130, 16), (70, 24), (3, 40)):
        SPECS.append(Spec("reparam_kl_fwd-B%d-D%d-coef" % (B, D), "dvae_reparam_kl_fwd", _reparam_fwd(B, D, "coef")))
    for nb, D in ((1, 10), (3, 1), (375, 16)):
        def finish(al, nb=nb, D=D):
            kl = al.inout("kl_dim", R((16 + nb * 16,), 5).abs())
            return [kl, nb, al.inp("coef", coef_vec(0.01)), D, stream()]
        SPECS.append(Spec("kl_finish-blocks%d-D%d" % (nb, D), "dvae_kl_finish", finish))
    opt = ("dz", "dz2", "dz3", "dmu_x", "dlv_x", "eps")
    for B, D, null in [(1, 10, None), (7, 10, "dz"), (130, 10, "dz2"), (200, 16, "dz3"), (33, 1, "dmu_x"), (1500, 10, "dlv_x"),
                       (70, 24, "eps")]:
        def rbwd(al, B=B, D=D, null=null):
            t = {k: (None if k == null else al.inp(k, R((B, D), 3 + i))) for i, k in enumerate(opt)}
            mu, lv = al.inp("mu", R((B, D), 20)), al.inp("logvar", R((B, D), 21, 0.7))
            scal = torch.zeros(_lib.nscal(D))
            scal[_lib.S_KLW] = 2.5
            return [t["dz"], t["dz2"], t["dz3"], t["dmu_x"], t["dlv_x"], mu, lv, t["eps"], al.inp("scal", scal),
                    al.inp("coef", coef_vec(1.0 / B)), al.out("dml", (B, 2 * D)), B, D, stream()]
        SPECS.append(Spec("reparam_kl_bwd-B%d-D%d-null-%s" % (B, D, null), "dvae_reparam_kl_bwd", rbwd))
    for B, D in ((1, 10), (7, 1), (1280, 16), (300, 24)):
        def klbwd(al, B=B, D=D):
            return [al.inp("g_dim", R((D,), 1)), al.inp("mu", R((B, D), 2)), al.inp("logvar", R((B, D), 3, 0.7)),
                    al.out("dmu", (B, D)), al.out("dlogvar", (B, D)), B, D, stream()]
        SPECS.append(Spec("kl_normal_bwd-B%d-D%d" % (B, D), "dvae_kl_normal_bwd", klbwd))


_latent_specs()


def _rowstats_mask(Bl, D):
    # include/dvae_hip.h: "DVAE_ROWSTATS 32: floats per row of the estimator's row statistics: 4 + D used"
    m = torch.zeros(Bl, _lib.rowstats_stride(D), dtype=torch.bool)
    m[:, :4 + D] = True
    return m


def _tc_inputs(Bg, D):
    mu, lv, eps = R((Bg, D), 1), R((Bg, D), 2, 0.7) - 0.5, R((Bg, D), 3, 1.5)
    z = mu + torch.exp(0.5 * lv) * eps
    lw = torch.zeros(4)
    from disvae_amd.utils.math import log_importance_weights
    lw[:3] = log_importance_weights(Bg, 5000)
    return z, mu, lv, lw


@functools.lru_cache(maxsize=16)
def _tc_forward(Bg, D, row0, Bl, mss):
    """(tmp, rowstats) of a forward call on ordinary device tensors: the inputs of dvae_btcvae_bwd (unused rowstats columns 0)."""
    z, mu, lv, lw = _tc_inputs(Bg, D)
    d = lambda t: t.to("cuda")
    zd, md, ld, lwd = d(z), d(mu), d(lv), d(lw)
    tmp = torch.zeros(_lib.btcvae_tmp_floats(Bg, Bl, D), device="cuda")
    rs = torch.zeros(Bl, _lib.rowstats_stride(D), device="cuda")
    _lib.call("dvae_btcvae_fwd", zd.data_ptr(), md.data_ptr(), ld.data_ptr(), Bg, D, row0, Bl, mss, lwd.data_ptr(), tmp.data_ptr(),
              rs.data_ptr(), stream())
    torch.cuda.synchronize()
    return tmp.cpu(), rs.cpu()


def _btcvae_specs():
    for Bg, D, row0, Bl, mss in [(8, 10, 0, 8, 1), (4, 10, 0, 4, 0), (70, 1, 0, 70, 1), (130, 16, 0, 130, 1), (300, 10, 150, 150, 1),
                                 (1030, 10, 0, 1030, 1), (64, 17, 0, 64, 1), (100, 40, 37, 63, 1), (2, 10, 1, 1, 1)]:
        gid = "Bg%d-D%d-row%d-Bl%d-mss%d" % (Bg, D, row0, Bl, mss)

        def fwd(al, Bg=Bg, D=D, row0=row0, Bl=Bl, mss=mss):
            z, mu, lv, lw = _tc_inputs(Bg, D)
            return [al.inp("z", z), al.inp("mu", mu), al.inp("logvar", lv), Bg, D, row0, Bl, mss, al.inp("log_w", lw),
                    al.ws("tmp", (_lib.btcvae_tmp_floats(Bg, Bl, D),)),
                    al.out("rowstats", (Bl, _lib.rowstats_stride(D)), written=_rowstats_mask(Bl, D)), stream()]
        SPECS.append(Spec("btcvae_fwd-" + gid, "dvae_btcvae_fwd", fwd))

        def bwd(al, Bg=Bg, D=D, row0=row0, Bl=Bl, mss=mss):
            z, mu, lv, lw = _tc_inputs(Bg, D)
            tmp, rs = _tc_forward(Bg, D, row0, Bl, mss)
            return [al.inp("z", z), al.inp("mu", mu), al.inp("logvar", lv), al.inp("rowstats", rs), Bg, D, row0, Bl, mss,
                    al.inp("log_w", lw), al.inp("coef", coef_vec(1.0 / Bg)), al.inp("tmp", tmp), al.out("dz", (Bl, D)),
                    al.out("dmu_all", (Bg, D)), al.out("dlv_all", (Bg, D)), stream()]
        SPECS.append(Spec("btcvae_bwd-" + gid, "dvae_btcvae_bwd", bwd))


_btcvae_specs()


def _scal_mask(D):
    # include/dvae_hip.h, "scalar slots written by dvae_loss_finalize": the DVAE_S_* enum names LOSS, REC, KL, KL0 .. KL0+D-1 (above
    # DVAE_MAX_D: DVAE_WIDE_KL0 + d), MI, TC, DWKL, KLW, DTC; the other slots of float[DVAE_NSCAL_D(D)] are not defined
    m = torch.zeros(_lib.nscal(D), dtype=torch.bool)
    for s in (_lib.S_LOSS, _lib.S_REC, _lib.S_KL, _lib.S_MI, _lib.S_TC, _lib.S_DWKL, _lib.S_KLW, _lib.S_DTC):
        m[s] = True
    m[_lib.kl0(D):_lib.kl0(D) + D] = True
    return m


def _loss_specs():
    kinds = [("betaH", _lib.LOSS_BETAH), ("betaB", _lib.LOSS_BETAB), ("btcvae", _lib.LOSS_BTCVAE), ("factor", _lib.LOSS_FACTOR)]
    for name, kind in kinds:
        for D, blocks, B in ((10, 0, 8), (10, 3, 700), (1, 375, 1500), (16, 1, 5), (24, 0, 70)):
            def common(al, D=D, blocks=blocks, B=B, kind=kind):
                parts = al.inp("rec_partials", R((_lib.REC_NPART,), 3).abs())
                nkl = D if D > _lib.MAX_LATENT_DIM else 16 + blocks * 16
                kl = al.inp("kl_dim", R((nkl,), 4).abs())
                rs = al.inp("rowstats", R((B, _lib.rowstats_stride(D)), 5)) if kind == _lib.LOSS_BTCVAE else None
                ds = al.inp("disc_sums", R((4,), 6)) if kind == _lib.LOSS_FACTOR else None
                return parts, kl, rs, ds

            def epi(al, D=D, blocks=blocks, B=B, kind=kind, common=common):
                parts, kl, rs, ds = common(al)
                return [kind, parts, kl, blocks, D, rs, B if rs is not None else 0, ds, B, al.inp("coef", coef_vec(1.0 / B)),
                        al.out("packed", (_lib.npack(D),)), al.out("scal", (_lib.nscal(D),), written=_scal_mask(D)), stream()]
            SPECS.append(Spec("loss_epilogue-%s-D%d-blocks%d-B%d" % (name, D, blocks, B), "dvae_loss_epilogue", epi))
            if blocks == 0:
                def pack(al, D=D, B=B, common=common):
                    parts, kl, rs, ds = common(al)
                    return [parts, kl, D, rs, B if rs is not None else 0, ds, al.out("packed", (_lib.npack(D),)), stream()]
                SPECS.append(Spec("loss_pack-%s-D%d-B%d" % (name, D, B), "dvae_loss_pack", pack))

                def fin(al, D=D, B=B, kind=kind):
                    return [kind, al.inp("packed", R((_lib.npack(D),), 7).abs()), D, B, al.inp("coef", coef_vec(1.0 / B)),
                            al.out("scal", (_lib.nscal(D),), written=_scal_mask(D)), stream()]
                SPECS.append(Spec("loss_finalize-%s-D%d-B%d" % (name, D, B), "dvae_loss_finalize", fin))

    @spec("loss_epilogue-pack-only", "dvae_loss_epilogue")
    def pack_only(al):
        return [_lib.LOSS_BETAH, al.inp("rec_partials", R((_lib.REC_NPART,), 3).abs()), al.inp("kl_dim", R((16,), 4).abs()), 0, 10, None, 0,
                None, 8, al.inp("coef", coef_vec()), al.out("packed", (_lib.NPACK,)), None, stream()]

    for B, D in ((1, 10), (37, 10), (1280, 16), (300, 24)):
        def perm(al, B=B, D=D):
            p = torch.stack([torch.randperm(B, generator=torch.Generator().manual_seed(d)) for d in range(D)])
            return [al.inp("z", R((B, D), 1)), al.inp("perm", p), al.out("out", (B, D)), B, D, stream()]
        SPECS.append(Spec("permute_dims-B%d-D%d" % (B, D), "dvae_permute_dims", perm))
    for Bh, tc in ((1, True), (50, True), (700, False), (33, True)):
        def disc(al, Bh=Bh, tc=tc):
            return [al.inp("dlogits", R((2 * Bh, 2), 2, 3.0)), Bh, al.inp("coef", coef_vec()), al.out("sums", (4,)),
                    al.out("g_dtc", (2 * Bh, 2)), al.out("g_tc", (Bh, 2)) if tc else None, stream()]
        SPECS.append(Spec("disc_losses-Bh%d-%s" % (Bh, "tc" if tc else "notc"), "dvae_disc_losses", disc))
    for q, (dist, n, with_g, logit) in enumerate([(0, 4, True, 1), (1, 4, True, 0), (2, 4, False, 1), (0, 1280, True, 0), (1, 1280, False, 1),
                                                  (2, 1280, True, 1), (0, 73728, True, 1), (1, 73728, True, 1), (2, 73732, True, 0),
                                                  (0, 2048 * 4 + 4, False, 1)]):
        def rloss(al, dist=dist, n=n, with_g=with_g, logit=logit):
            return [al.inp("recon", U((n,), 1) * 0.98 + 0.01), al.inp("target", U((n,), 2)), n, dist, al.inp("coef", coef_vec()),
                    al.out("partials", (_lib.REC_NPART,)), al.out("g", (n,)) if with_g else None, logit, stream()]
        SPECS.append(Spec("recon_loss-dist%d-n%d-%s-logit%d" % (dist, n, "g" if with_g else "nog", logit), "dvae_recon_loss", rloss))
    for n in (1, 7, 1280, 65537):
        def sbwd(al, n=n):
            return [al.inp("grad_y", R((n,), 1)), al.inp("y", U((n,), 2)), al.out("out", (n,)), n, stream()]
        SPECS.append(Spec("sigmoid_bwd-n%d" % n, "dvae_sigmoid_bwd", sbwd))

        def rsum(al, n=n):
            return [al.inp("src", R((n,), 1)), n, 0.125, al.out("dst", (1,)), stream()]
        SPECS.append(Spec("reduce_sum-n%d" % n, "dvae_reduce_sum", rsum))

    @spec("set_coef", "dvae_set_coef")
    def set_coef(al):
        return [al.out("coef", (_lib.NCOEF,)), 0.5, 1.5, 2.5, 3.5, 4.5, 5.5, 6.5, 7.5, stream()]


_loss_specs()


# ===== glue =====================================================================================================================
def _glue_specs():
    for n in (1, 7, 1280, 65537):
        def add(al, n=n):
            return [al.inp("a", R((n,), 1)), al.inp("b", R((n,), 2)), al.out("out", (n,)), n, stream()]
        SPECS.append(Spec("add-n%d" % n, "dvae_add", add))

        def add_alias(al, n=n):
            a = al.inout("a", R((n,), 1))
            return [a, al.inp("b", R((n,), 2)), a, n, stream()]
        SPECS.append(Spec("add-inplace-n%d" % n, "dvae_add", add_alias))

        def axpby(al, n=n):
            return [al.out("out", (n,)), al.inp("a", R((n,), 1)), 0.125, al.inp("b", R((n,), 2)), 7.0, n, stream()]
        SPECS.append(Spec("axpby-n%d" % n, "dvae_axpby", axpby))

        def axpby_nob(al, n=n):
            return [al.out("out", (n,)), al.inp("a", R((n,), 1)), 3.0, None, 0.0, n, stream()]
        SPECS.append(Spec("axpby-no-b-n%d" % n, "dvae_axpby", axpby_nob))

        def axpby_alias_a(al, n=n):
            a = al.inout("a", R((n,), 1))
            return [a, a, 1.0, al.inp("b", R((n,), 2)), 7.0, n, stream()]
        SPECS.append(Spec("axpby-out-is-a-n%d" % n, "dvae_axpby", axpby_alias_a))

        def axpby_alias_b(al, n=n):
            b = al.inout("b", R((n,), 2))
            return [b, al.inp("a", R((n,), 1)), 0.5, b, 2.0, n, stream()]
        SPECS.append(Spec("axpby-out-is-b-n%d" % n, "dvae_axpby", axpby_alias_b))

        def u8f(al, n=n):
            return [al.inp("src", BYTES((n,), 1)), al.out("dst", (n,)), n, stream()]        # "both 16-byte aligned"
        SPECS.append(Spec("u8_to_f32-n%d" % n, "dvae_u8_to_f32", u8f))
    for A, Bn, inner in ((8, 3, 1280), (2, 8, 1280), (3, 5, 7), (1, 4, 33), (4, 1, 10), (1, 1, 1), (2, 1, 65537)):
        def swap(al, A=A, Bn=Bn, inner=inner):
            return [al.inp("src", R((A, Bn, inner), 1)), al.out("dst", (Bn, A, inner)), A, Bn, inner, stream()]
        SPECS.append(Spec("swap_outer-%d-%d-%d" % (A, Bn, inner), "dvae_swap_outer", swap))
    for N, C, H in ((1, 32, 4), (5, 32, 4), (33, 32, 4), (70, 32, 8), (3, 3, 6), (2, 1, 2)):
        for src in (NCHW, NHWC):
            def relay(al, N=N, C=C, H=H, src=src):
                return [al.inp("src", R(act(N, C, H, src), 1)), src, al.out("dst", act(N, C, H, NHWC if src == NCHW else NCHW)), N, C, H, H,
                        stream()]
            SPECS.append(Spec("relayout-N%d-C%d-H%d-from-%s" % (N, C, H, "nchw" if src == NCHW else "nhwc"), "dvae_relayout", relay))


_glue_specs()


# ===== the rest =================================================================================================================
@spec("adam_step-five-odd-tensors", "dvae_adam_step")
def _adam(al):
    lens = (1, 7, 1283, 65537, 33)
    arr = al.keep((_lib.AdamTensor * len(lens))())
    for q, (d, n) in enumerate(zip(arr, lens)):
        d.p = al.inout("p%d" % q, R((n,), 1 + q)).ptr
        d.g = al.inp("g%d" % q, R((n,), 11 + q)).ptr
        d.m = al.inout("m%d" % q, R((n,), 21 + q, 0.1)).ptr
        d.v = al.inout("v%d" % q, R((n,), 31 + q, 0.1).abs()).ptr
        d.step = None if q == 2 else al.out("step%d" % q, (1,)).ptr
        d.n = n
    return [ctypes.addressof(arr), len(lens), 4.0, 5e-4, 0.9, 0.999, 1e-8, 0.01, stream()]


def _rest_specs():
    for N, D, S in ((50, 10, 33), (1000, 3, 7), (1, 1, 1), (300, 20, 500)):
        def ent(al, N=N, D=D, S=S):
            nws = int(_lib.lib().dvae_latent_entropy_ws_floats(N, D, S))
            return [al.inp("z_ds", R((D, S), 1)), al.inp("mean", R((N, D), 2)), al.inp("logvar", R((N, D), 3, 0.7)), N, D, S,
                    al.ws("ws", (nws,)), al.out("H", (D,)), stream()]
        SPECS.append(Spec("latent_entropy-N%d-D%d-S%d" % (N, D, S), "dvae_latent_entropy", ent))
    for u8 in (0, 1):
        for K in (1, 17):
            for row in (1000, 12288):
                for n_img in (1, 5):
                    def rows(al, u8=u8, K=K, row=row, n_img=n_img):
                        need = ctypes.c_long()
                        _lib.call("dvae_recon_rows_ws_floats", n_img, K, row, ctypes.addressof(need))
                        recon = al.inp("recon", U((n_img * K, row), 1) * 0.98 + 0.01)
                        # dvae_recon_rows: "uint8 pixels (target_u8 != 0, 4-byte aligned ...)"
                        tgt = al.inp("target", BYTES((n_img, row), 2), align=4) if u8 else al.inp("target", U((n_img, row), 2))
                        ws = al.ws("ws", (need.value,)) if need.value else None
                        return [recon, tgt, u8, n_img, K, row, (K + row) % 3, ws, al.out("rec_rows", (n_img * K,)), stream()]
                    SPECS.append(Spec("recon_rows-%s-K%d-row%d-n%d" % ("u8" if u8 else "f32", K, row, n_img), "dvae_recon_rows", rows))
    for first, last in ((1, 0), (0, 0), (0, 1), (1, 1)):
        for n_img, nk, D in ((1, 1, 10), (5, 17, 10), (130, 3, 24)):
            def iw(al, first=first, last=last, n_img=n_img, nk=nk, D=D):
                mu, lv = al.inp("mu", R((n_img, D), 1)), al.inp("logvar", R((n_img, D), 2, 0.7))
                z, eps = al.inp("z", R((n_img * nk, D), 3)), al.inp("eps", R((n_img * nk, D), 4))
                rec = al.inp("rec_rows", R((n_img * nk,), 5).abs() * 100)
                if first:
                    state = al.out("state", (n_img, 2))       # "first != 0 starts it"
                else:
                    st = torch.stack((R((n_img,), 6) * 10, R((n_img,), 7).abs() + 1.0), dim=1)
                    state = al.inout("state", st)
                loglik = al.out("loglik", (n_img,)) if last else None
                kl = al.out("kl", (n_img, D)) if (first + last) == 1 else None
                return [mu, lv, z, eps, rec, n_img, nk, D, 3 * nk, first, last, state, loglik, kl, stream()]
            SPECS.append(Spec("iw_loglik-first%d-last%d-n%d-nk%d-D%d" % (first, last, n_img, nk, D), "dvae_iw_loglik", iw))
    for n_img, D in ((1, 10), (130, 24)):
        def iw_kl(al, n_img=n_img, D=D):
            return [al.inp("mu", R((n_img, D), 1)), al.inp("logvar", R((n_img, D), 2, 0.7)), None, None, None, n_img, 1, D, 1, 1, 1, None,
                    None, al.out("kl", (n_img, D)), stream()]
        SPECS.append(Spec("iw_loglik-kl-only-n%d-D%d" % (n_img, D), "dvae_iw_loglik", iw_kl))
    for n, C, H, nrow, pad, up in ((1, 1, 7, 8, 2, 1), (1, 3, 8, 8, 2, 3), (5, 1, 7, 3, 2, 1), (5, 3, 9, 2, 1, 2), (5, 3, 64, 8, 2, 1)):
        def grid(al, n=n, C=C, H=H, nrow=nrow, pad=pad, up=up):
            gh, gw = ctypes.c_long(), ctypes.c_long()
            _lib.call("dvae_image_grid_shape", n, H, H, nrow, pad, up, ctypes.addressof(gh), ctypes.addressof(gw))
            # dvae_image_grid_u8: "out holds gh * gw * 3 bytes (written with 16-byte stores when it is 16-byte aligned)": any alignment
            return [al.inp("imgs", U((n, C, H, H), 1) * 1.2 - 0.1), n, C, H, H, nrow, pad, 0.5, up,
                    al.out("out", (gh.value, gw.value, 3), dtype=U8, align=1), stream()]
        SPECS.append(Spec("image_grid_u8-n%d-C%d-H%d-nrow%d-pad%d-up%d" % (n, C, H, nrow, pad, up), "dvae_image_grid_u8", grid))


_rest_specs()


def test_image_grid_cases_include_a_size_that_is_no_multiple_of_16():
    sizes = []
    for n, H, nrow, pad, up in ((1, 7, 8, 2, 1), (5, 7, 3, 2, 1), (5, 9, 2, 1, 2)):
        gh, gw = ctypes.c_long(), ctypes.c_long()
        _lib.call("dvae_image_grid_shape", n, H, H, nrow, pad, up, ctypes.addressof(gh), ctypes.addressof(gw))
        sizes.append(gh.value * gw.value * 3)
    assert any(s % 16 for s in sizes), sizes


@pytest.mark.parametrize("spec", SPECS, ids=[s.id for s in SPECS])
def test_memory_contract(spec):
    with force_generic(spec.generic):
        run_contract(spec.entry, spec.build, contract=spec.id)


# ===== the harness sees device-side traffic =====================================================================================
# n = payload + 1: one element past the tensors.  37 floats = 148 bytes: the extra element of the PLAIN run stays inside the
# 512-byte block the allocator rounds the tensor to, the extra element of the guarded runs is guard memory this test owns.
def test_device_write_one_past_the_end_is_seen_as_a_back_guard_write():
    n = 37

    def build(al):
        return [al.inp("a", R((n,), 1)), al.inp("b", R((n,), 2)), al.out("out", (n,)), n + 1, stream()]
    with pytest.raises(GuardError) as ei:
        run_contract("dvae_add", build)
    e = ei.value
    assert (e.arg, e.side, e.offset, e.count) == ("out", "back guard", n, 1), str(e)


def test_device_read_one_past_the_end_is_seen_in_the_result():
    n = 37

    def build(al):
        return [al.inp("src", R((n,), 1)), n + 1, 1.0, al.out("dst", (1,)), stream()]
    with pytest.raises(GuardError) as ei:
        run_contract("dvae_reduce_sum", build)
    e = ei.value
    assert e.arg == "dst" and e.side in ("differing bits", "non-finite output") and e.offset == 0, str(e)
