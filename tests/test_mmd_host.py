"""CPU: the host side of the InfoVAE / MMD-VAE loss -- the fp64 restatement (tests/mmd_ref.py) against a literal double loop over
the pairs and against torch autograd, the tenth library's C-ABI (include/dvae_mmd_hip.h == disvae_amd/_mmdlib.py == the built
libdvae_mmd_hip.so), its row of build.py's PLUGIN_TARGETS (and TARGETS untouched), the rules its source obeys, the keys
get_loss_f reads, the refusal of data-parallel steps before any device work, and e32: the ratio error / bound that an fp32 numpy
restatement attains on the tables and shapes of the GPU tests (tests/test_gpu_mmd.py multiplies the fp32 part of its gradient
bound by max(1, 4 e32)).

e32, measured on the CPU over mmd_ref.TABLES x KERNELS x B in SHAPES_B x D in SHAPES_D (mmd_ref.fp32_gradients: every operation
in fp32): the worst is printed by test_e32_is_what_was_measured and pinned in mmd_ref.E32_WORST within a factor of 2 either way
(numpy builds differ in their summation order).
"""
import ctypes
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import mmd_ref as R
import disvae_amd
from disvae_amd import _cabi, _diplib, _lib, _mmdlib
from disvae_amd.models import losses as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dvae_mmd_hip.h")
CSRC = os.path.join(ROOT, "disentangling-vae_amd", "csrc")
TRIP_Z = _mmdlib.COLS * _mmdlib.MAX_CGROUPS // 2          # the last B whose z tiles make one trip (2 B columns)
TRIP_P = _mmdlib.COLS * _mmdlib.MAX_CGROUPS               # ... whose p tiles make one trip (B columns)
# the shapes of tests/test_gpu_mmd.py: one row on either side of ROWS (a second row tile; 2 B crosses COLS there as well), of COLS
# (a second column chunk of a p tile) and of both first second trips
SHAPES_B = (1, 2, 3, 33, _mmdlib.ROWS, _mmdlib.ROWS + 1, _mmdlib.COLS, TRIP_Z, TRIP_Z + 1, TRIP_P, TRIP_P + 1)
SHAPES_D = (1, 2, 10, 16, 17, 40, 128)


def _build():
    spec = importlib.util.spec_from_file_location("dvae_build_mmd", os.path.join(ROOT, "disentangling-vae_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- 1. the restatement -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.KERNELS)
@pytest.mark.parametrize("tab", R.TABLES)
def test_restatement_is_the_literal_double_loop(tab, kind):
    for B, D in ((1, 3), (2, 1), (5, 4), (12, 10)):
        z, p, mu = R.table(tab, B, D)
        h = R.default_bandwidth(D)
        ref = R.mmd(z, p, kind, h, 3.0, mu)
        val, g = R.mmd_literal(z, p, kind, h)
        scale = (abs(ref["S_zz"]) + abs(ref["S_pp"]) + abs(ref["S_zp"])) / (B * B) + 1e-300
        assert abs(ref["mmd"] - val) <= 1e-13 * scale, (B, D)
        assert np.abs(ref["dz"] - g).max() <= 1e-11 * (ref["gabs"].max() + 1e-300), (B, D)       # (the shift by z_0 costs the offset table |p - z_0| u)
        assert ref["wmmd"] == 3.0 * ref["mmd"] and np.array_equal(ref["dmu"], 3.0 * ref["dz"])
        assert np.array_equal(ref["dlv"], ref["dmu"] * (0.5 * (z.astype(np.float64) - mu.astype(np.float64))))


@pytest.mark.parametrize("kind", R.KERNELS)
@pytest.mark.parametrize("tab", R.TABLES)
def test_analytic_gradients_are_autograds(tab, kind):
    for B, D, h in ((2, 3, None), (5, 1, 0.7), (33, 10, None), (40, 17, 50.0)):
        z, p, mu = R.table(tab, B, D)
        h = R.default_bandwidth(D) if h is None else h
        ref = R.mmd(z, p, kind, h)
        tz = torch.tensor(z, dtype=torch.float64, requires_grad=True)
        val = R.regulariser_torch(tz, torch.tensor(p, dtype=torch.float64), kind, h)
        (gz,) = torch.autograd.grad(val, [tz])
        scale = (abs(ref["S_zz"]) + abs(ref["S_pp"]) + abs(ref["S_zp"])) / (B * B) + 1e-300
        assert abs(val.item() - ref["mmd"]) <= 1e-12 * scale
        assert np.abs(gz.numpy() - ref["dz"]).max() <= 1e-12 * (ref["gabs"].max() + 1e-300)


@pytest.mark.parametrize("kind", R.KERNELS)
def test_one_row_gives_zero(kind):
    z, p, mu = R.table("gauss", 1, 4)
    ref = R.mmd(z, p, kind, 8.0, 999.0, mu)
    assert ref["mmd"] == 0.0 and ref["wmmd"] == 0.0 and ref["S_zz"] == 0.0 and ref["S_pp"] == 0.0 and ref["S_zp"] > 0.0
    assert not ref["dz"].any() and not ref["dmu"].any() and not ref["dlv"].any()
    tz = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    val = R.regulariser_torch(tz, torch.tensor(p, dtype=torch.float64), kind, 8.0)
    assert val.item() == 0.0 and not torch.autograd.grad(val, [tz])[0].any()
    assert R.mmd_literal(z, p, kind, 8.0)[0] == 0.0


def test_the_norm_expansion_fails_the_offset_table_and_differences_do_not():
    z, p, mu = R.table("offset", 64, 10)
    ref = R.mmd(z, p, "imq", 20.0)
    tol = R.tolerances(ref)
    bad = R.mmd_norm_expansion(z, p, "imq", 20.0)
    assert abs(bad - ref["S_zz"]) > 10 * tol["S_zz"]                        # (r^2 ~ 2e-5 there; an ulp of |z|^2 is 1e-3)
    k, _ = R.kernel(R._r2(z, z, np.float32), "imq", 20.0)                  # fp32 differences stay inside the bound
    good = float((k.astype(np.float64) * ~np.eye(64, dtype=bool)).sum())
    assert abs(good - ref["S_zz"]) <= tol["S_zz"]


def test_e32_is_what_was_measured():
    worst, where = 0.0, None
    for tab in R.TABLES:
        for kind in R.KERNELS:
            for B in SHAPES_B:
                for D in SHAPES_D:
                    v = R.e32(tab, B, D, kind)
                    if v > worst:
                        worst, where = v, (tab, kind, B, D)
    print("e32 = %.4g at %r (pinned %.4g)" % (worst, where, R.E32_WORST))
    assert R.E32_WORST / 2 <= worst <= R.E32_WORST * 2
    assert R.MARGIN == max(1.0, 4 * R.E32_WORST)


# ---- 2. the library -----------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _nm(path, *flags):
    nm = shutil.which("nm") or shutil.which("llvm-nm", path="/opt/rocm/llvm/bin")
    assert nm, "no nm on this machine"
    return subprocess.run([nm] + list(flags) + [path], capture_output=True, text=True, check=True).stdout


def test_header_ctypes_table_and_exports_agree(monkeypatch):
    declared = sorted(set(re.findall(r"\b(dvae_mmd_[a-zA-Z0-9_]+)\s*\(", _header())))
    assert declared == sorted(_mmdlib.SIGNATURES)
    assert declared == sorted(["dvae_mmd_version", "dvae_mmd_last_error", "dvae_mmd_ws_doubles", "dvae_mmd_pairs", "dvae_mmd_finish"])
    exported = sorted(set(re.findall(r" T (dvae_\w+)", _nm(os.path.abspath(_mmdlib.LIB_PATH), "-D", "--defined-only"))))
    assert exported == declared
    assert re.findall(r" U (dvae_\w+)", _nm(os.path.abspath(_mmdlib.LIB_PATH), "-D")) == []
    kinds = {ctypes.c_void_p: "p", ctypes.c_int: "i", ctypes.c_long: "l", ctypes.c_double: "d"}
    for name, params in re.findall(r"\b(dvae_mmd_[a-zA-Z0-9_]+)\s*\(([^)]*)\)", _header()):
        got = []
        for prm in [x.strip() for x in params.split(",") if x.strip() != "void"]:
            got.append("p" if "*" in prm else ("l" if prm.startswith("long") else ("d" if prm.startswith("double") else "i")))
        assert got == [kinds[t] for t in _mmdlib.SIGNATURES[name]], name
    macros = {k: int(v) for k, v in re.findall(r"#define (DVAE_MMD_\w+) (\d+)", _header())}
    mirrored = {"DVAE_MMD_VERSION": _mmdlib.VERSION, "DVAE_MMD_MAX_D": _mmdlib.MAX_D, "DVAE_MMD_MAX_B": _mmdlib.MAX_B,
                "DVAE_MMD_RBF": _mmdlib.RBF, "DVAE_MMD_IMQ": _mmdlib.IMQ, "DVAE_MMD_THREADS": _mmdlib.THREADS,
                "DVAE_MMD_ROWS": _mmdlib.ROWS, "DVAE_MMD_COLS": _mmdlib.COLS, "DVAE_MMD_MAX_CGROUPS": _mmdlib.MAX_CGROUPS}
    assert macros == mirrored                                            # every macro of the header, none besides
    assert _mmdlib.MAX_D == 128 and _mmdlib.KERNELS == {"rbf": 0, "imq": 1} and _mmdlib.IMQ_SCALES == R.SCALES
    assert _mmdlib.lib().dvae_mmd_version() == _mmdlib.VERSION == 1
    assert os.path.basename(_mmdlib.LIB_PATH) == "libdvae_mmd_hip.so"
    binding = open(_mmdlib.__file__).read()
    assert 'Binding.for_library("mmd", SIGNATURES, _RESTYPE' in binding and "LIB_PATH = _binding.path" in binding
    assert _mmdlib._binding.last_error == "dvae_mmd_last_error" and _mmdlib._binding.signatures is _mmdlib.SIGNATURES
    monkeypatch.setenv("DVAE_MMD_HIP_LIB", "/elsewhere/lib.so")              # the override, read when a binding is made
    assert _cabi.Binding.for_library("mmd", {}, {}, "").path == "/elsewhere/lib.so"
    assert "InfoVaeLoss" in disvae_amd.__all__ and disvae_amd.InfoVaeLoss is L.InfoVaeLoss
    # k_mmd_pairs' LDS at the largest D: rows and a trip's columns in fp64 at an odd stride, c in fp32, the waves' sums
    assert 8 * (_mmdlib.ROWS + _mmdlib.COLS) * (_mmdlib.MAX_D + 1) + 4 * _mmdlib.ROWS * (_mmdlib.COLS + 1) + 64 <= 64 * 1024


def test_workspace_sizes_and_the_tiling_mirror():
    h = _mmdlib.lib()
    for B in SHAPES_B + (31, 64, 65, 1024, 4097, _mmdlib.MAX_B):
        for D in (1, 10, 128):
            assert h.dvae_mmd_ws_doubles(B, D) == _mmdlib.ws_doubles(B, D) >= 4 + B * D, (B, D)
        tiles, (gz, cz), (gp, cp) = _mmdlib.tiling(B)
        assert tiles == -(-B // _mmdlib.ROWS)
        assert gp <= gz <= _mmdlib.MAX_CGROUPS and gz * cz >= 2 * B > (gz - 1) * cz and gp * cp >= B > (gp - 1) * cp
        assert (-(-cz // _mmdlib.COLS) > 1) == (B > TRIP_Z) and (-(-cp // _mmdlib.COLS) > 1) == (B > TRIP_P)
    assert _mmdlib.tiling(_mmdlib.ROWS)[0] == 1 and _mmdlib.tiling(_mmdlib.ROWS + 1)[0] == 2
    assert _mmdlib.tiling(_mmdlib.ROWS)[1][0] == 1 and _mmdlib.tiling(_mmdlib.ROWS + 1)[1][0] == 2      # 2 B crosses COLS
    assert _mmdlib.tiling(_mmdlib.COLS)[2][0] == 1 and _mmdlib.tiling(_mmdlib.COLS + 1)[2][0] == 2
    bad = ((0, 3), (-1, 3), (5, 0), (5, _mmdlib.MAX_D + 1), (_mmdlib.MAX_B + 1, 3))
    assert [h.dvae_mmd_ws_doubles(*a) for a in bad] == [0] * 5
    assert h.dvae_mmd_ws_doubles(_mmdlib.MAX_B, _mmdlib.MAX_D) > 0 and _mmdlib.OUT_DOUBLES == 5


def test_build_has_the_plugin_row_and_targets_is_unchanged():
    build = _build()
    assert [tuple(row) for row in build.PLUGIN_TARGETS] == [("mmd", ["mmd_pairs"], "dvae_mmd_hip.h")]
    assert [n for n, _s, _h in build.TARGETS] == ["", "eval", "score", "info", "irs", "unsup", "udr", "dci", "dip"]
    assert "mmd_pairs" not in build.ALL_SOURCES and len(build.ALL_SOURCES) == 31
    assert build.MMD_SOURCES == ["mmd_pairs"] and os.path.exists(os.path.join(build.SRC, "mmd_pairs.hip"))
    assert os.path.basename(build.MMD_LIB) == "libdvae_mmd_hip.so" and os.path.exists(build.MMD_LIB)
    assert os.path.dirname(os.path.abspath(build.MMD_LIB)) == os.path.join(ROOT, "disentangling-vae_amd", "lib")
    assert sorted(os.path.basename(h) for h in build.MMD_HEADERS if "include" in h.split(os.sep)) == ["dvae_hip.h", "dvae_mmd_hip.h"]
    assert {os.path.basename(h) for h in build.MMD_HEADERS} - {"dvae_hip.h", "dvae_mmd_hip.h"} == \
        {f for f in os.listdir(CSRC) if f.endswith(".h")}
    assert build._target(*build.PLUGIN_TARGETS[0])[3] == os.path.join(build.OBJ, "flags_mmd.txt")
    text = open(os.path.join(ROOT, "disentangling-vae_amd", "build.py")).read()
    assert "for name, sources, header in TARGETS + PLUGIN_TARGETS:" in text               # one loop, the same FLAGS and stamp logic
    src = open(os.path.join(CSRC, "mmd_pairs.hip")).read()
    assert sorted(re.findall(r'^#include "([^"]+)"', src, re.M)) == ["../../include/dvae_mmd_hip.h", "common.h", "last_error.h", "table_stats.h"]


def test_source_obeys_the_rules_of_the_shared_plumbing():
    src = open(os.path.join(CSRC, "mmd_pairs.hip")).read()
    assert len(re.findall(r'^#include "last_error\.h"', src, re.M)) == 1
    assert not re.search(r"\bthread_local\b", src) and not re.search(r"^void set_error\(", src, re.M)
    for name in ("put_f64", "get_f64", "chunks_of", "lesser"):
        assert not re.search(r"^[ \w]*\b(?:void|double|int|T)\s+%s\s*\([^;{]*\)\s*\{" % name, src, re.M), name
    code = src.split("#include", 1)[1]
    assert not re.search(r"atomic", code)                                   # no atomics of any kind
    assert "while" not in code and "hipLaunchCooperativeKernel" not in src  # no spinning, no cooperative launch
    assert not re.search(r"hipMalloc|hipFree|hipMemcpy|hipMemset|Synchronize", src)    # the entry points only enqueue
    assert not re.search(r"1\.837877|0\.9189385|6\.2831853", src)
    assert len(re.findall(r"hipLaunchKernelGGL\(", src)) == 2               # one launch per entry point: two per step
    # r^2 from the differences: no dot product of two rows, no squared norms
    assert re.search(r"df = a\[d\] - b\[d\];\s*r2 = fma\(df, df, r2\);", code) and not re.search(r"norm|a\[d\] \* b\[d\]", code)


def test_call_raises_with_the_librarys_own_error_text():
    h = _mmdlib.lib()
    dummy = 1 << 20                                                # aligned non-NULL address, never dereferenced
    #        z      p      B   D  kernel h    grad ws     stream
    pairs = [dummy, dummy, 60, 3, 1,     6.0, 1,   dummy, None]
    #         z      mu     B   D  w      ws     dmu    dlv    out    loss_io stream
    finish = [dummy, dummy, 60, 3, 999.0, dummy, dummy, dummy, dummy, None, None]

    def put(good, i, v):
        return good[:i] + [v] + good[i + 1:]
    bad = [("dvae_mmd_pairs", put(pairs, i, None)) for i in (0, 1, 7)] + [("dvae_mmd_finish", put(finish, i, None)) for i in (5, 8)]
    for name, good in (("dvae_mmd_pairs", pairs), ("dvae_mmd_finish", finish)):
        bad += [(name, put(good, 2, 0)), (name, put(good, 2, -1)), (name, put(good, 2, _mmdlib.MAX_B + 1)), (name, put(good, 3, 0)),
                (name, put(good, 3, _mmdlib.MAX_D + 1))]
    bad += [("dvae_mmd_pairs", put(pairs, 4, 2)), ("dvae_mmd_pairs", put(pairs, 4, -1))]                   # no such kernel
    bad += [("dvae_mmd_pairs", put(pairs, 5, v)) for v in (0.0, -1.0, float("nan"), float("inf"))]       # the bandwidth
    bad += [("dvae_mmd_finish", put(finish, 4, v)) for v in (float("nan"), float("inf"))]                # the weight
    bad += [("dvae_mmd_finish", put(finish, i, None)) for i in (0, 1, 6)]                                 # dlv without z, mu or dmu
    for name, args in bad:
        with pytest.raises(_lib.DvaeHipError) as e:
            _mmdlib.call(name, *args)
        own = h.dvae_mmd_last_error().decode()
        assert "invalid argument" in own and "mmd_pairs.hip" in own, (name, args, own)
        assert str(e.value) == "%s failed (-1): %s" % (name, own)
    assert "mmd_pairs.hip" not in _diplib.lib().dvae_dip_last_error().decode()         # every library keeps its own buffer


def test_call_loads_through_the_modules_lib(monkeypatch):
    class Boom(Exception):
        pass

    def boom():
        raise Boom("lib() of the module was asked")
    monkeypatch.setattr(_mmdlib, "lib", boom)
    with pytest.raises(Boom, match="was asked"):
        _mmdlib.call("dvae_mmd_pairs", 1 << 20, 1 << 20, 4, 3, 0, 6.0, 0, 1 << 20, None)


# ---- 3. the loss plugin ---------------------------------------------------------------------------------------------------------
HP = dict(rec_dist="bernoulli", reg_anneal=10000, betaH_B=4, betaB_initC=0, betaB_finC=25, betaB_G=1000, factor_G=6.4,
          latent_dim=10, lr_disc=1e-4, btcvae_A=1, btcvae_B=6.4, btcvae_G=1, n_data=1000)


def test_get_loss_f_keys_and_defaults():
    assert L.INFO_LOSSES == ["infovae"] and L.DIP_LOSSES == ["dipI", "dipII"] and L.LOSSES == ["VAE", "betaH", "betaB", "factor", "btcvae"]
    f = L.get_loss_f("infovae", device="cpu", **HP)
    assert isinstance(f, L.InfoVaeLoss) and f.KIND == _lib.LOSS_BETAH
    assert (f.alpha, f.lam, f.kernel, f.bandwidth, f.beta, f.weight) == (0.0, 1000.0, "imq", None, 1.0, 999.0)
    assert f.steps_anneal == 10000 and f.rec_dist == "bernoulli"
    assert f._h(10) == 20.0 == R.default_bandwidth(10)
    assert f._coefs(False) == dict(ANNEAL=1, BETA=1.0)
    g = L.get_loss_f("infovae", device="cpu", info_alpha=1.0, info_lambda=250.0, mmd_kernel="rbf", mmd_bandwidth=3.5, **HP)
    assert (g.alpha, g.lam, g.kernel, g.bandwidth, g.beta, g.weight, g._h(10)) == (1.0, 250.0, "rbf", 3.5, 0.0, 250.0, 3.5)   # MMD-VAE
    assert [k for k, _ in g.STORED] == ["recon_loss", "kl_loss", "mmd_loss", "loss"] and dict(g.STORED)["mmd_loss"] is None
    assert L.InfoVaeLoss(alpha=-2.0, lam=0.5).weight == -2.5               # any finite weight
    with pytest.raises(ValueError):
        L.InfoVaeLoss(kernel="laplace")
    with pytest.raises(ValueError):
        L.InfoVaeLoss(bandwidth=0.0)
    with pytest.raises(ValueError):
        L.get_loss_f("infoVAE2", device="cpu", **HP)
    assert f._replay_key.__func__ is L.InfoVaeLoss._replay_key             # kernel, bandwidth, alpha and lam join the replay key

    with pytest.raises(ValueError, match="latent_sample"):
        f(torch.zeros(2, 1, 32, 32), torch.zeros(2, 1, 32, 32), (torch.zeros(2, 10), torch.zeros(2, 10)), True, None)
    assert f.n_train_steps == 0


class _Comm:
    world_size, rank = 2, 0


def test_data_parallel_steps_are_refused_before_any_device_work(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("device work before the refusal")
    monkeypatch.setattr(_mmdlib, "lib", boom)
    monkeypatch.setattr(_lib, "lib", boom)
    monkeypatch.setattr(L, "call", boom)
    f = L.get_loss_f("infovae", device="cpu", **HP)
    f.comm = _Comm()

    class _Model:
        training = True
        latent_dim = 10

        @property
        def engine(self):
            boom()
    with pytest.raises(NotImplementedError, match="all_gather_latents"):
        f.fused_step(torch.zeros(4, 1, 32, 32), _Model(), None, None)
    assert f.n_train_steps == 0
