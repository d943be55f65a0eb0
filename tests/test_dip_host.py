"""CPU: the host side of the DIP-VAE I / II losses -- the fp64 restatement (tests/dip_ref.py) against the literal
disentanglement_lib form and numpy.cov, its analytic gradients against torch autograd, the ninth library's C-ABI
(include/dvae_dip_hip.h == disvae_amd/_diplib.py == the built libdvae_dip_hip.so), its row of build.py's TARGETS, the keys
get_loss_f reads, the refusal of data-parallel steps before any device work, and e32: the ratio error / bound that an fp32 numpy
restatement attains on the tables and shapes of the GPU tests (tests/test_gpu_dip.py multiplies its fp32 bound by
max(1, 4 e32)).

e32, measured on the CPU over dip_ref.TABLES x TYPES x B in SHAPES_B x D in SHAPES_D (dip_ref.fp32_gradients: the gradient stage
in fp32 on operands rounded once from fp64): the worst is printed by test_e32_is_what_was_measured and pinned in
dip_ref.E32_WORST within a factor of 2 either way (BLAS builds differ in their summation order).
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

import dip_ref as R
import disvae_amd
from disvae_amd import _cabi, _diplib, _lib, _dcilib
from disvae_amd.models import losses as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dvae_dip_hip.h")
CSRC = os.path.join(ROOT, "disentangling-vae_amd", "csrc")
# the shapes of tests/test_gpu_dip.py: one row on either side of BLOCK_ROWS and of BLOCK_ROWS * MAX_GROUPS (the second trip)
SHAPES_B = (1, 2, 3, 33, _diplib.BLOCK_ROWS, _diplib.BLOCK_ROWS * _diplib.MAX_GROUPS, _diplib.BLOCK_ROWS * _diplib.MAX_GROUPS + 1)
SHAPES_D = (1, 2, 10, 16, 17, 40, 128)


def _build():
    spec = importlib.util.spec_from_file_location("dvae_build_dip", os.path.join(ROOT, "disentangling-vae_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- 1. the restatement -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dip_type", R.TYPES)
@pytest.mark.parametrize("kind", ("gauss", "regime"))
def test_restatement_is_the_literal_form_and_numpys_cov(kind, dip_type):
    for B, D in ((1, 3), (2, 1), (33, 10), (257, 17)):
        mu, lv = R.table(kind, B, D)
        C = R.covariance(mu, lv, dip_type)
        lit = R.covariance_literal(mu, lv, dip_type)
        scale = (mu.astype(np.float64) ** 2).mean(axis=0)
        tol = 16 * R.U * np.sqrt(scale[:, None] * scale[None, :]) * B + 1e-300      # the literal form cancels raw moments
        assert (np.abs(C - lit) <= tol).all()
        cov = np.cov(mu.astype(np.float64).T, bias=True).reshape(D, D)
        if dip_type == "ii":
            cov = cov + np.diag(np.exp(lv.astype(np.float64)).mean(axis=0))
        assert np.abs(C - cov).max() <= 1e-12 * max(1.0, np.abs(cov).max())
        assert np.array_equal(C, C.T) or np.abs(C - C.T).max() <= 1e-15 * np.abs(C).max()
    mu, lv = R.table("gauss", 1, 4)
    assert not R.covariance(mu, lv, "i").any()                                        # one row: no spread


@pytest.mark.parametrize("dip_type", R.TYPES)
@pytest.mark.parametrize("kind", R.TABLES)
def test_analytic_gradients_are_autograds(kind, dip_type):
    for B, D, lam_od, lam_d in ((1, 3, 10.0, 100.0), (5, 1, 2.0, 3.0), (33, 10, 10.0, 10.0), (64, 17, 5.0, 50.0)):
        mu, lv = R.table(kind, B, D)
        ref = R.regulariser(mu, lv, dip_type, lam_od, lam_d)
        tmu = torch.tensor(mu, dtype=torch.float64, requires_grad=True)
        tlv = torch.tensor(lv, dtype=torch.float64, requires_grad=True)
        Rt = R.regulariser_torch(tmu, tlv, dip_type, lam_od, lam_d)
        gmu, glv = torch.autograd.grad(Rt, [tmu, tlv], allow_unused=True)
        assert abs(Rt.item() - ref["R"]) <= 1e-12 * max(1.0, abs(ref["R"]))
        assert abs(ref["R"] - ref["R_od"] - ref["R_d"]) <= 1e-15 * max(1.0, abs(ref["R"]))
        s = np.abs(ref["dmu"]).max() + 1e-300
        assert np.abs(gmu.numpy() - ref["dmu"]).max() <= 1e-12 * s
        if dip_type == "ii":
            assert np.abs(glv.numpy() - ref["dlv"]).max() <= 1e-12 * (np.abs(ref["dlv"]).max() + 1e-300)
        else:
            assert glv is None and ref["dlv"] is None
        if D == 1:
            assert ref["R_od"] == 0.0                                                  # no off-diagonal pair


def test_a_raw_moment_fp32_sum_fails_the_offset_family_and_fp64_shifted_does_not():
    mu, lv = R.table("offset", 256, 10)
    ref = R.regulariser(mu, lv, "i", 10.0, 100.0)
    tol = R.tolerances(ref, 10.0, 100.0)["C"]
    raw = R.fp32_raw_moment_cov(mu)
    assert np.abs(raw - ref["C"]).max() > 1e3 * tol.max() and np.abs(raw - ref["C"]).max() > 10 * np.abs(ref["C"]).max()
    x = mu.astype(np.float64) - mu[0].astype(np.float64)                               # the device's order, in fp64
    s1 = x.sum(axis=0) / 256
    shifted = x.T @ x / 256 - np.outer(s1, s1)
    assert (np.abs(shifted - ref["C"]) <= tol).all()


def test_e32_is_what_was_measured():
    worst, where = 0.0, None
    for kind in R.TABLES:
        for dip_type in R.TYPES:
            for B in SHAPES_B:
                for D in SHAPES_D:
                    v = R.e32(kind, B, D, dip_type)
                    if v > worst:
                        worst, where = v, (kind, dip_type, B, D)
    print("e32 = %.4g at %r (pinned %.4g)" % (worst, where, R.E32_WORST))
    assert R.E32_WORST / 2 <= worst <= R.E32_WORST * 2


# ---- 2. the library -----------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _nm(path, *flags):
    nm = shutil.which("nm") or shutil.which("llvm-nm", path="/opt/rocm/llvm/bin")
    assert nm, "no nm on this machine"
    return subprocess.run([nm] + list(flags) + [path], capture_output=True, text=True, check=True).stdout


def test_header_ctypes_table_and_exports_agree(monkeypatch):
    declared = sorted(set(re.findall(r"\b(dvae_dip_[a-zA-Z0-9_]+)\s*\(", _header())))
    assert declared == sorted(_diplib.SIGNATURES)
    assert declared == sorted(["dvae_dip_version", "dvae_dip_last_error", "dvae_dip_ws_doubles", "dvae_dip_moments", "dvae_dip_grad"])
    exported = sorted(set(re.findall(r" T (dvae_\w+)", _nm(os.path.abspath(_diplib.LIB_PATH), "-D", "--defined-only"))))
    assert exported == declared
    kinds = {ctypes.c_void_p: "p", ctypes.c_int: "i", ctypes.c_long: "l", ctypes.c_double: "d"}
    for name, params in re.findall(r"\b(dvae_dip_[a-zA-Z0-9_]+)\s*\(([^)]*)\)", _header()):
        got = []
        for prm in [x.strip() for x in params.split(",") if x.strip() != "void"]:
            got.append("p" if "*" in prm else ("l" if prm.startswith("long") else ("d" if prm.startswith("double") else "i")))
        assert got == [kinds[t] for t in _diplib.SIGNATURES[name]], name
    macros = {k: int(v) for k, v in re.findall(r"#define (DVAE_DIP_\w+) (\d+)", _header())}
    mirrored = {"DVAE_DIP_VERSION": _diplib.VERSION, "DVAE_DIP_MAX_D": _diplib.MAX_D, "DVAE_DIP_THREADS": _diplib.THREADS,
                "DVAE_DIP_BLOCK_ROWS": _diplib.BLOCK_ROWS, "DVAE_DIP_MAX_GROUPS": _diplib.MAX_GROUPS}
    assert macros == mirrored                                            # every macro of the header, none besides
    assert _diplib.MAX_D == 128 and 2 * _diplib.MAX_D <= _diplib.THREADS
    assert _diplib.lib().dvae_dip_version() == _diplib.VERSION == 1
    assert os.path.basename(_diplib.LIB_PATH) == "libdvae_dip_hip.so"
    binding = open(_diplib.__file__).read()
    assert 'Binding.for_library("dip", SIGNATURES, _RESTYPE' in binding and "LIB_PATH = _binding.path" in binding
    assert _diplib._binding.last_error == "dvae_dip_last_error" and _diplib._binding.signatures is _diplib.SIGNATURES
    monkeypatch.setenv("DVAE_DIP_HIP_LIB", "/elsewhere/lib.so")              # the override, read when a binding is made
    assert _cabi.Binding.for_library("dip", {}, {}, "").path == "/elsewhere/lib.so"
    assert "DipVaeLoss" in disvae_amd.__all__ and disvae_amd.DipVaeLoss is L.DipVaeLoss
    # k_dip_grad's LDS at the largest D: G fp32 [D, D], the centred rows of a trip and two vectors in fp64 -- within a CDNA4 compute unit
    D = _diplib.MAX_D
    assert 4 * D * D + 8 * D * (_diplib.BLOCK_ROWS + 2) <= 160 * 1024


def test_workspace_sizes_and_the_chunking_mirror():
    h = _diplib.lib()
    for B in SHAPES_B + (31, 64, 65, 4096, 4097, 100000):
        for D in (1, 10, 128):
            assert h.dvae_dip_ws_doubles(B, D) == _diplib.ws_doubles(B, D) >= 2 * D + D * D, (B, D)
        groups, chunk = _diplib.groups(B)
        assert groups <= _diplib.MAX_GROUPS and groups * chunk >= B > (groups - 1) * chunk
        trips = -(-chunk // _diplib.BLOCK_ROWS)
        assert (trips > 1) == (B > _diplib.BLOCK_ROWS * _diplib.MAX_GROUPS)
    assert _diplib.groups(_diplib.BLOCK_ROWS)[0] == 1 and _diplib.groups(_diplib.BLOCK_ROWS + 1)[0] == 2
    assert [h.dvae_dip_ws_doubles(*a) for a in ((0, 3), (-1, 3), (5, 0), (5, _diplib.MAX_D + 1), (2 ** 31, 3))] == [0] * 5
    assert _diplib.out_doubles(10) == 103


def test_build_table_has_the_dip_row():
    build = _build()
    assert ("dip", ["dip_cov"], "dvae_dip_hip.h") in [tuple(row) for row in build.TARGETS]
    names = [n for n, _s, _h in build.TARGETS]
    assert len(names) == len(set(names)) >= 9                             # nine libraries (the next one is one more row)
    others = {s for n, sources, _h in build.TARGETS if n != "dip" for s in sources}
    assert "dip_cov" not in others and build.DIP_SOURCES == ["dip_cov"]
    assert os.path.basename(build.DIP_LIB) == "libdvae_dip_hip.so" and os.path.exists(build.DIP_LIB)
    assert sorted(os.path.basename(h) for h in build.DIP_HEADERS if "include" in h.split(os.sep)) == ["dvae_dip_hip.h", "dvae_hip.h"]
    assert {os.path.basename(h) for h in build.DIP_HEADERS} - {"dvae_hip.h", "dvae_dip_hip.h"} == \
        {f for f in os.listdir(CSRC) if f.endswith(".h")}
    assert "dip_cov" in build.ALL_SOURCES                                  # tools/isa_identity.py compares it
    # nothing of another library is linked in or included
    src = open(os.path.join(CSRC, "dip_cov.hip")).read()
    assert sorted(re.findall(r'^#include "([^"]+)"', src, re.M)) == ["../../include/dvae_dip_hip.h", "common.h", "last_error.h", "table_stats.h"]
    undefined = re.findall(r" U (dvae_\w+)", _nm(os.path.abspath(_diplib.LIB_PATH), "-D"))
    assert undefined == []


def test_source_obeys_the_rules_of_the_shared_plumbing():
    src = open(os.path.join(CSRC, "dip_cov.hip")).read()
    assert len(re.findall(r'^#include "last_error\.h"', src, re.M)) == 1
    assert not re.search(r"\bthread_local\b", src) and not re.search(r"^void set_error\(", src, re.M)
    for name in ("put_f64", "get_f64", "chunks_of", "lesser"):
        assert not re.search(r"^[ \w]*\b(?:void|double|int|T)\s+%s\s*\([^;{]*\)\s*\{" % name, src, re.M), name
    assert not re.search(r"atomic", src.split("#include", 1)[1])            # no atomics of any kind
    assert "while" not in src and "hipLaunchCooperativeKernel" not in src   # no spinning, no cooperative launch
    assert not re.search(r"hipMalloc|hipFree|hipMemcpy|hipMemset|Synchronize", src)    # the entry points only enqueue
    assert not re.search(r"1\.837877|0\.9189385|6\.2831853", src)


def test_call_raises_with_the_librarys_own_error_text():
    h = _diplib.lib()
    dummy = 1 << 20                                                # aligned non-NULL address, never dereferenced
    #          mu     logvar  B  D  ws     stream
    moments = [dummy, dummy, 60, 3, dummy, None]
    #       mu     logvar  B  D  l_od  l_d   ws     dmu    dlv    out    loss_io stream
    grad = [dummy, dummy, 60, 3, 10.0, 10.0, dummy, dummy, dummy, dummy, None, None]

    def put(good, i, v):
        return good[:i] + [v] + good[i + 1:]
    bad = [("dvae_dip_moments", put(moments, i, None)) for i in (0, 4)] + [("dvae_dip_grad", put(grad, i, None)) for i in (0, 6, 9)]
    for name, good in (("dvae_dip_moments", moments), ("dvae_dip_grad", grad)):
        bad += [(name, put(good, 2, 0)), (name, put(good, 2, -1)), (name, put(good, 3, 0)), (name, put(good, 3, _diplib.MAX_D + 1))]
    bad.append(("dvae_dip_grad", put(grad, 1, None)))               # dlv without logvar
    bad.append(("dvae_dip_grad", put(grad, 7, None)))               # dlv without dmu
    for name, args in bad:
        with pytest.raises(_lib.DvaeHipError) as e:
            _diplib.call(name, *args)
        own = h.dvae_dip_last_error().decode()
        assert "invalid argument" in own and "dip_cov.hip" in own, (name, args, own)
        assert str(e.value) == "%s failed (-1): %s" % (name, own)
    assert "dip_cov.hip" not in _dcilib.lib().dvae_dci_last_error().decode()         # every library keeps its own buffer


# ---- 3. the loss plugin ---------------------------------------------------------------------------------------------------------
HP = dict(rec_dist="bernoulli", reg_anneal=10000, betaH_B=4, betaB_initC=0, betaB_finC=25, betaB_G=1000, factor_G=6.4,
          latent_dim=10, lr_disc=1e-4, btcvae_A=1, btcvae_B=6.4, btcvae_G=1, n_data=1000)


def test_get_loss_f_keys_and_defaults():
    assert L.DIP_LOSSES == ["dipI", "dipII"] and L.LOSSES == ["VAE", "betaH", "betaB", "factor", "btcvae"]
    for name, dip_type, factor in (("dipI", "i", 10.0), ("dipII", "ii", 1.0)):
        f = L.get_loss_f(name, device="cpu", **HP)
        assert isinstance(f, L.DipVaeLoss) and f.KIND == _lib.LOSS_BETAH and f.beta == 1
        assert (f.dip_type, f.lambda_od, f.lambda_d_factor, f.lambda_d) == (dip_type, 10.0, factor, 10.0 * factor)
        assert f.steps_anneal == 10000 and f.rec_dist == "bernoulli"
        assert R.default_lambda_d_factor(dip_type) == factor
        g = L.get_loss_f(name, device="cpu", dip_lambda_od=2.5, dip_lambda_d_factor=4.0, **HP)
        assert (g.lambda_od, g.lambda_d_factor, g.lambda_d) == (2.5, 4.0, 10.0)
        assert [k for k, _ in g.STORED] == ["recon_loss", "kl_loss", "dip_loss", "loss"]
    with pytest.raises(ValueError):
        L.DipVaeLoss(dip_type="iii")
    with pytest.raises(ValueError):
        L.get_loss_f("dipIII", device="cpu", **HP)
    a, b = L.DipVaeLoss("i"), L.DipVaeLoss("i", lambda_od=11.0)
    key = lambda f: f._replay_key.__func__ is L.DipVaeLoss._replay_key
    assert key(a) and key(b)                                            # lambda_od, lambda_d and dip_type join the replay key


class _Comm:
    world_size, rank = 2, 0


def test_data_parallel_steps_are_refused_before_any_device_work(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("device work before the refusal")
    monkeypatch.setattr(_diplib, "lib", boom)
    monkeypatch.setattr(_lib, "lib", boom)
    monkeypatch.setattr(L, "call", boom)
    f = L.get_loss_f("dipII", device="cpu", **HP)
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
