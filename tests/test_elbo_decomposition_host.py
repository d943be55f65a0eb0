"""CPU: the host side of the data-set level ELBO decomposition -- the fp64 restatement (tests/decomp_ref.py) against closed
forms, the second library's C-ABI (include/dvae_eval_hip.h == disvae_amd/_evallib.py == the built libdvae_eval_hip.so), the
build, and the argument errors Evaluator.compute_elbo_decomposition raises before any device work."""
import ctypes
import importlib
import importlib.util
import math
import os
import re
import shutil
import subprocess

import pytest
import torch

import decomp_ref as R
from disvae_amd import _evallib, _lib, Evaluator
from disvae_amd.models.losses import get_loss_f
from disvae_amd.models.vae import init_specific_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dvae_eval_hip.h")
NEW_KERNELS = ("k_joint_prep", "k_joint_lse", "k_joint_lse_wide", "k_joint_finish", "k_sample_terms", "k_eval_means")
HP = dict(rec_dist="bernoulli", reg_anneal=0, betaH_B=4, betaB_initC=0, betaB_finC=25, betaB_G=1000, factor_G=6.4,
          latent_dim=4, lr_disc=1e-4, btcvae_A=1, btcvae_B=6.4, btcvae_G=1)


# ---- 1. the restatement against closed forms ---------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,S", [(7, 3, 5), (50, 10, 50), (1, 1, 1)])
def test_identical_standard_normal_posteriors_decompose_to_zero(N, D, S):
    """Every q(z|x_n) = N(0, I): q(z) = N(0, I) = p(z) exactly, z = eps, so the three terms vanish sample by sample."""
    gen = torch.Generator().manual_seed(N)
    mean, logvar = torch.zeros(N, D, dtype=torch.float64), torch.zeros(N, D, dtype=torch.float64)
    rows = torch.randperm(N, generator=gen)[:S]
    eps = torch.randn(S, D, generator=gen, dtype=torch.float64)
    ref = R.decomposition(R.sample_z(mean, logvar, rows, eps), eps, rows, mean, logvar)
    for k in ("mi", "tc", "dw_kl", "kl"):
        assert abs(ref[k]) <= 1e-12, (k, ref[k])
    assert ref["n_samples"] == S and ref["n_data"] == N


def test_one_dimension_has_no_total_correlation_and_the_terms_add_up():
    gen = torch.Generator().manual_seed(3)
    N, S = 40, 25
    mean, logvar = torch.randn(N, 1, generator=gen).double(), (torch.rand(N, 1, generator=gen) - 1).double()
    rows = torch.randperm(N, generator=gen)[:S]
    eps = torch.randn(S, 1, generator=gen).double()
    ref = R.decomposition(R.sample_z(mean, logvar, rows, eps), eps, rows, mean, logvar)
    assert ref["tc"] == 0.0                                      # D = 1: the joint IS the marginal, bit for bit
    assert ref["mi"] > 0 and ref["kl"] == ref["mi"] + ref["tc"] + ref["dw_kl"]
    mean, logvar, rows, eps = R.clustered_posteriors(300, 6, 70, seed=1)
    assert rows.shape == (70,) and eps.shape == (70, 6) and rows.unique().numel() == 70
    assert R.clustered_posteriors(9, 10, 257, seed=1)[2].shape == (257,)          # S > N: rows repeat
    ref = R.decomposition(R.sample_z(mean, logvar, rows, eps), eps, rows, mean, logvar)
    assert ref["kl"] == ref["mi"] + ref["tc"] + ref["dw_kl"]
    # ... and the sum is the sampled KL itself: 1/S sum_s [log q(z_s | x_n(s)) - log p(z_s)]
    assert ref["kl"] == pytest.approx((ref["logqz_condx"] - ref["logpz"]).mean().item(), rel=1e-12)
    assert ref["tc"] > 0 and 0 < ref["mi"] < math.log(300)


# ---- 2. the library -----------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _nm(path, *flags):
    nm = shutil.which("nm") or shutil.which("llvm-nm", path="/opt/rocm/llvm/bin")
    assert nm, "no nm on this machine"
    return subprocess.run([nm] + list(flags) + [path], capture_output=True, text=True, check=True).stdout


def test_header_ctypes_table_and_exports_agree():
    declared = sorted(set(re.findall(r"\b(dvae_eval_[a-zA-Z0-9_]+)\s*\(", _header())))
    assert declared == sorted(_evallib.SIGNATURES) and len(declared) == 5
    exported = sorted(set(re.findall(r" T (dvae_\w+)", _nm(os.path.abspath(_evallib.LIB_PATH), "-D", "--defined-only"))))
    assert exported == declared
    # parameter counts and kinds: pointers / int / long of every declaration as the table has them
    kinds = {ctypes.c_void_p: "p", ctypes.c_int: "i", ctypes.c_long: "l"}
    for name, params in re.findall(r"\b(dvae_eval_[a-zA-Z0-9_]+)\s*\(([^)]*)\)", _header()):
        got = []
        for prm in [x.strip() for x in params.split(",") if x.strip() != "void"]:
            got.append("p" if "*" in prm else ("l" if prm.startswith("long") else "i"))
        assert got == [kinds[t] for t in _evallib.SIGNATURES[name]], name
    macros = dict(re.findall(r"#define (DVAE_EVAL_\w+) (\d+)", _header()))
    assert int(macros["DVAE_EVAL_VERSION"]) == _evallib.VERSION == 1 == _evallib.lib().dvae_eval_version()
    assert int(macros["DVAE_EVAL_JOINT_CHUNK"]) == _evallib.JOINT_CHUNK
    assert int(macros["DVAE_EVAL_JOINT_MAX_CHUNKS"]) == _evallib.JOINT_MAX_CHUNKS


def test_argument_errors_are_reported_before_any_launch():
    h = _evallib.lib()
    dummy = 1 << 20                                               # aligned non-NULL address, never dereferenced
    joint = [dummy, dummy, dummy, 5, 3, 4, dummy, dummy, dummy, None]
    terms = [dummy, dummy, dummy, dummy, 5, 3, 4, dummy, dummy, dummy, None]
    bad = []
    for name, good, ptrs, sizes in (("dvae_eval_joint_logq", joint, (0, 1, 2, 6, 7, 8), (3, 4, 5)),
                                    ("dvae_eval_sample_terms", terms, (0, 1, 2, 3, 7, 8, 9), (4, 5, 6))):
        for i in ptrs:
            bad.append((name, good[:i] + [None] + good[i + 1:]))
        for i in sizes:
            bad.append((name, good[:i] + [0] + good[i + 1:]))
            bad.append((name, good[:i] + [-1] + good[i + 1:]))
    for name, args in bad:
        with pytest.raises(_lib.DvaeHipError, match="invalid argument"):
            _evallib.call(name, *args)
        assert b"invalid argument" in h.dvae_eval_last_error()


def test_workspace_size_is_zero_for_empty_problems_and_monotone():
    ws = _evallib.lib().dvae_eval_joint_logq_ws_floats
    for N, D, S in ((0, 10, 5), (5, 0, 5), (5, 10, 0), (-1, 10, 5), (5, -3, 5), (5, 10, -7)):
        assert ws(N, D, S) == 0
    L = _evallib.JOINT_CHUNK
    sizes = [1, 2, 7, 255, 256, 257, 1000, L - 1, L, L + 1, 10000, 10240, 10241, 65536, 100000, 737280, 1 << 22]
    for D in (1, 4, 5, 10, 16, 17, 33):
        for a in sizes:
            row = [ws(a, D, b) for b in sizes]
            col = [ws(b, D, a) for b in sizes]
            assert row == sorted(row) and col == sorted(col), (D, a)
            assert row[0] >= a * (2 * D + 1) + 2                  # the record table and one (max, sum) pair at the least
    assert ws(737280, 10, 737280) * 4 < 1 << 30                   # the paper's S = N estimate of dSprites: under 1 GiB


# ---- 3. the build -------------------------------------------------------------------------------------------------------------
def test_build_leaves_both_libraries_and_keeps_them_apart():
    g = importlib.import_module("__graft_entry__")
    g.build()
    main, ev = os.path.abspath(_lib.LIB_PATH), os.path.abspath(_evallib.LIB_PATH)
    assert os.path.dirname(main) == os.path.dirname(ev) and os.path.exists(main) and os.path.exists(ev)
    assert os.path.basename(ev) == "libdvae_eval_hip.so"
    spec = importlib.util.spec_from_file_location("dvae_build_again", os.path.join(ROOT, "disentangling-vae_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert "elbo_decomp" not in mod.SOURCES and mod.EVAL_SOURCES == ["elbo_decomp"]
    assert os.path.abspath(mod.build(verbose=False)) == main      # still the training library's path
    in_main, in_eval = _nm(main, "-C"), _nm(ev, "-C")
    for k in NEW_KERNELS:
        assert not re.search(r"\b%s\b" % k, in_main), k + " is in libdvae_hip.so"
        assert re.search(r"__device_stub__%s\b" % k, in_eval), k + " is not in libdvae_eval_hip.so"
    assert "dvae_eval_" not in in_main
    assert _lib.lib().dvae_version() == 109


# ---- 4. Evaluator: errors before any device work -------------------------------------------------------------------------------
def test_evaluator_argument_errors():
    model = init_specific_model("Burgess", (1, 32, 32), 4)              # on the CPU: any device work would raise DvaeHipError
    ev = Evaluator(model, get_loss_f("VAE", **HP), device=torch.device("cpu"), is_progress_bar=False)
    loader = [(torch.rand(2, 1, 32, 32), None), (torch.rand(3, 1, 32, 32), None)]
    with pytest.raises(ValueError, match="n_samples=6 exceeds the 5 images"):
        ev.compute_elbo_decomposition(loader, n_samples=6)
    with pytest.raises(ValueError, match="n_samples must be >= 1"):
        ev.compute_elbo_decomposition(loader, n_samples=0)
    with pytest.raises(ValueError, match=r"eps must have shape \(3, 4\)"):
        ev.compute_elbo_decomposition(loader, n_samples=3, eps=torch.zeros(3, 5))
    with pytest.raises(ValueError, match=r"eps must have shape \(5, 4\)"):
        ev.compute_elbo_decomposition(loader, n_samples=None, eps=torch.zeros(4, 4))
    with pytest.raises(ValueError, match=r"sample_idx must hold rows in \[0, 5\)"):
        ev.compute_elbo_decomposition(loader, sample_idx=[0, 5])
    with pytest.raises(ValueError, match="exceeds"):
        ev.compute_elbo_decomposition(loader, sample_idx=[0, 1, 2, 3, 4, 0])

    class Sized:                                                        # a DataLoader: the data set's length is asked first
        dataset = list(range(5))

        def __iter__(self):
            raise AssertionError("iterated before the sizes were checked")
    with pytest.raises(ValueError, match="exceeds"):
        ev.compute_elbo_decomposition(Sized(), n_samples=10000)
    model.train()
    with pytest.raises(_lib.DvaeHipError):                              # valid arguments: the native encoder refuses the CPU
        ev.compute_elbo_decomposition(loader, n_samples=2)
    assert model.training                                               # ... and the mode is as it was
