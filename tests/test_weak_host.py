"""CPU: the host side of the weakly-supervised pair losses Ada-GVAE / Ada-ML-VAE -- the fp64 restatement of the adaptive group
posterior (tests/weak_ref.py) against closed forms and the literal product of experts, its torch form against the numpy one, the
oracle of a whole pair step against the plain VAE oracle, the library's C-ABI (include/dvae_weak_hip.h == disvae_amd/_weaklib.py
== the built lib_scores/libdvae_weak_hip.so) and its row of build.py's SCORE_TARGETS, the loss surface (WEAK_LOSSES, get_loss_f,
the exports, the three refusals before any device work, __call__), draw_pair_partners / PairedFactorLoader, and the band: on the
two table families of the GPU tests no entry lies within it and a numpy float32 evaluation flips no mask bit against float64.
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

import weak_ref as R
import disvae_amd
from disvae_amd import _cabi, _lib, _weaklib, _dcilib
from disvae_amd import data as DATA
from disvae_amd.models import losses as L
from oracle import disvae_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dvae_weak_hip.h")
CSRC = os.path.join(ROOT, "disentangling-vae_amd", "csrc")


def _build():
    spec = importlib.util.spec_from_file_location("dvae_build_weak", os.path.join(ROOT, "disentangling-vae_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- 1. the restatement -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
def test_closed_forms(kind):
    rng = np.random.RandomState(3)
    P, D = 7, 10
    mu, lv = R.table("gauss", P, D)
    # an identical pair: every delta is exactly 0, nothing is shared, the operator is the identity
    mu_i, lv_i = np.concatenate([mu[:P], mu[:P]]), np.concatenate([lv[:P], lv[:P]])
    out = R.aggregate(mu_i, lv_i, kind)
    assert not out["delta"].any() and not out["shared"].any()
    assert np.array_equal(out["mu"], mu_i.astype(np.float64)) and np.array_equal(out["lv"], lv_i.astype(np.float64))
    # ... and where it IS aggregated, the group posterior of two equal posteriors is that posterior
    assert np.abs(out["m"] - mu_i[:P]).max() <= 1e-15 and np.abs(out["lvt"] - lv_i[:P]).max() <= 4e-15
    # D = 1: max = min = tau, nothing is shared
    out = R.aggregate(mu[:, :1], lv[:, :1], kind)
    assert not out["shared"].any() and np.array_equal(out["mu"], mu[:, :1].astype(np.float64))
    assert np.array_equal(out["tau"], out["delta"][:, 0])
    # equal variances: the mean of variances and the product of experts coincide (w = 1 / 2)
    lv_e = np.concatenate([lv[:P], lv[:P]])
    a, b = R.aggregate(mu, lv_e, "gvae"), R.aggregate(mu, lv_e, "mlvae")
    assert a["shared"].any() and np.array_equal(a["shared"], b["shared"])
    assert np.abs(a["mu"] - b["mu"]).max() <= 1e-15 and np.abs(a["lv"] - b["lv"]).max() <= 4e-15
    # one far dimension: all others are shared
    far = rng.randint(0, D, P)
    mu_f, lv_f = mu_i.copy(), lv_i.copy()
    mu_f[P:] += 1e-3 * rng.randn(P, D).astype(np.float32)
    mu_f[P + np.arange(P), far] += 5.0
    out = R.aggregate(mu_f, lv_f, kind)
    want = np.ones((P, D), dtype=bool)
    want[np.arange(P), far] = False
    assert np.array_equal(out["shared"], want)
    assert np.array_equal(out["mu"][:P][want], out["mu"][P:][want]) and np.array_equal(out["lv"][:P][want], out["lv"][P:][want])
    assert np.array_equal(out["mu"][:P][~want], mu_f[:P][~want].astype(np.float64))
    assert np.array_equal(out["mu"][P:][~want], mu_f[P:][~want].astype(np.float64))
    # an infinite delta: tau is infinite and every finite dimension is shared; a NaN compares false
    d = np.array([[1.0, np.inf, 3.0], [np.nan, 1.0, 2.0], [np.nan, np.nan, np.nan]])
    tau, sh = R.mask_of(d)
    assert tau[0] == np.inf and sh.tolist() == [[True, False, True], [False, True, False], [False, False, False]]


def test_mlvae_is_the_literal_product_of_experts_and_gvae_the_mean_of_variances():
    for family in R.FAMILIES:
        mu, lv = R.table(family, 33, 10)
        out = R.aggregate(mu, lv, "mlvae")
        m, lvt = R.mlvae_literal(mu, lv)
        assert np.abs(out["lvt"] - lvt).max() <= 1e-14 * max(1.0, np.abs(lvt).max())
        assert np.abs(out["m"] - m).max() <= 1e-14 * max(1.0, np.abs(m).max())
        out = R.aggregate(mu, lv, "gvae")
        ma, la, mb, lb = R.split(mu.astype(np.float64), lv.astype(np.float64))
        lit = np.log(0.5 * (np.exp(la) + np.exp(lb)))
        assert np.abs(out["lvt"] - lit).max() <= 1e-14 * max(1.0, np.abs(lit).max())
        assert np.array_equal(out["m"], 0.5 * (ma + mb))
        # delta is twice KL(q_a || q_b) per dimension
        kl = 0.5 * (np.exp(la - lb) + (mb - ma) ** 2 / np.exp(lb) - 1.0 + lb - la)
        assert np.abs(out["delta"] - 2 * kl).max() <= 1e-12 * np.abs(kl).max()
    words = R.bits_of(out["shared"])
    assert words.dtype == np.uint64 and np.array_equal(R.unbits(words, 10), out["shared"])
    assert np.array_equal(R.unbits(words.view(np.int64), 10), out["shared"])
    full = np.ones((2, 64), dtype=bool)
    assert R.bits_of(full).tolist() == [2 ** 64 - 1] * 2 and R.unbits(R.bits_of(full), 64).all()


@pytest.mark.parametrize("kind", R.KINDS)
def test_torch_form_is_the_numpy_form_and_takes_the_mask_as_an_input(kind):
    mu, lv = R.table("gauss", 9, 6)
    out = R.aggregate(mu, lv, kind)
    tmu = torch.tensor(mu, dtype=torch.float64, requires_grad=True)
    tlv = torch.tensor(lv, dtype=torch.float64, requires_grad=True)
    m, l = R.aggregate_torch(tmu, tlv, kind, out["shared"])
    assert np.abs(m.detach().numpy() - out["mu"]).max() <= 1e-15 and np.abs(l.detach().numpy() - out["lv"]).max() <= 4e-15
    flipped = ~out["shared"]
    m2, l2 = R.aggregate_torch(tmu, tlv, kind, flipped)
    other = R.aggregate(mu, lv, kind, shared=flipped)
    assert np.abs(m2.detach().numpy() - other["mu"]).max() <= 1e-15 and not np.array_equal(other["mu"], out["mu"])
    # the gradient: both rows of a shared element receive the pair's summed gradient, split as the header says
    gm, gl = torch.randn(18, 6, dtype=torch.float64), torch.randn(18, 6, dtype=torch.float64)
    dmu, dlv = torch.autograd.grad((m * gm).sum() + (l * gl).sum(), [tmu, tlv])
    sh = torch.tensor(out["shared"])
    Gm, Gl = gm[:9] + gm[9:], gl[:9] + gl[9:]
    t = (tlv[9:] - tlv[:9]).detach()
    wa, wb = torch.sigmoid(t), torch.sigmoid(-t)
    if kind == "gvae":
        want_mu = torch.cat([torch.where(sh, 0.5 * Gm, gm[:9]), torch.where(sh, 0.5 * Gm, gm[9:])])
        want_lv = torch.cat([torch.where(sh, Gl * wb, gl[:9]), torch.where(sh, Gl * wa, gl[9:])])
    else:
        c = Gm * wa * wb * (tmu[:9] - tmu[9:]).detach()
        want_mu = torch.cat([torch.where(sh, Gm * wa, gm[:9]), torch.where(sh, Gm * wb, gm[9:])])
        want_lv = torch.cat([torch.where(sh, Gl * wa - c, gl[:9]), torch.where(sh, Gl * wb + c, gl[9:])])
    assert (dmu - want_mu).abs().max() <= 1e-14 and (dlv - want_lv).abs().max() <= 1e-13
    # log-variances 40 apart: the small weight is 4e-18 and its gradient keeps its relative accuracy (sigmoid's own backward,
    # s (1 - s), returns 0 there)
    a = torch.tensor([[0.5], [-1.5]], dtype=torch.float64, requires_grad=True)
    v = torch.tensor([[-20.0], [20.0]], dtype=torch.float64, requires_grad=True)
    m, l = R.aggregate_torch(a, v, kind, np.ones((1, 1), dtype=bool))
    (dv,) = torch.autograd.grad(m[0, 0], [v], allow_unused=True)
    wb = 1.0 / (1.0 + np.exp(40.0))
    want = (1.0 - wb) * wb * 2.0
    if kind == "gvae":
        assert dv is None                                                  # the mean of means does not read the variances
    else:
        assert abs(dv[1, 0].item() - want) <= 1e-12 * want and abs(dv[0, 0].item() + want) <= 1e-12 * want

def test_the_step_oracle_with_an_empty_mask_is_the_vae_oracle():
    img, P, D = (1, 32, 32), 3, 10
    hp = dict(rec_dist="bernoulli", reg_anneal=10000, latent_dim=D)
    torch.manual_seed(5)
    p0 = O.init_vae_params(img, D)
    gen = torch.Generator().manual_seed(6)
    data, eps = torch.rand((2 * P,) + img, generator=gen).double(), torch.randn(2 * P, D, generator=gen).double()
    st = O.LossState(steps_anneal=10000); st.n_train_steps = 4
    want = O.train_iteration_grads("VAE", hp, st, O.clone_params(p0, dtype=torch.float64, requires_grad=True), data, eps)
    none = np.zeros((P, D), dtype=bool)
    for kind in R.KINDS:
        st = O.LossState(steps_anneal=10000); st.n_train_steps = 4
        got = R.weak_iteration_grads(kind, hp, st, O.clone_params(p0, dtype=torch.float64, requires_grad=True), data, eps, shared=none)
        assert got[0].item() == want[0].item() and st.n_train_steps == 5
        assert [k for k in got[1] if k != "shared_dims"] == list(want[1]) and got[1]["shared_dims"].item() == 0.0
        for k in want[2]:
            assert torch.equal(got[2][k], want[2][k]), k
        assert torch.equal(got[3]["mu"], want[3]["mu"]) and torch.equal(got[3]["recon"], want[3]["recon"])
        # its own mask aggregates something and changes the loss
        st = O.LossState(steps_anneal=10000); st.n_train_steps = 4
        own = R.weak_iteration_grads(kind, hp, st, O.clone_params(p0, dtype=torch.float64, requires_grad=True), data, eps)
        assert own[3]["shared"].any() and own[0].item() != want[0].item()
        assert 0 < own[1]["shared_dims"].item() < D
        assert torch.equal(own[3]["mu0"], want[3]["mu"])


# ---- 2. the band --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", R.FAMILIES)
def test_the_band_is_empty_on_the_test_families_and_fp32_flips_no_bit(family):
    for P, D in sorted(set(R.HOST_SIZES + R.GPU_SIZES)):
        mu, lv = R.table(family, P, D)
        band = R.band_of(mu, lv)
        own = R.aggregate(mu, lv, "gvae")["own"]
        flips = R.mask_fp32(mu, lv) != own
        print("%s P=%d D=%d: %d entries in the band, %d flips, %.2f shared dimensions per pair"
              % (family, P, D, band.sum(), flips.sum(), own.sum(axis=1).mean()))
        if D == 1:                                                         # delta = tau: the whole table is the band, and nothing is shared
            assert band.all() and not own.any() and not flips.any()
            continue
        assert not band.any(), (family, P, D)
        assert not flips.any(), (family, P, D)
        assert own.any() and not own.all(axis=1).any()                    # something is shared, never everything
    # the bounds of the GPU tests lie inside the band: even at the margin, delta's fp32 error is below BAND / 2 of its own scale
    mu, lv = R.table(family, 64, 10)
    T = np.abs(R.delta_terms(mu, lv)).sum(axis=0)
    assert (R.MARGIN * R.forward_bounds(mu, lv, "gvae")["delta"] <= 0.5 * R.BAND * T).all()


def test_edge_table_masks_are_what_its_docstring_says():
    for D in (1, 2, 10, 17, 64):
        mu, lv, expected = R.edge_table(D)
        for kind in R.KINDS:
            out = R.aggregate(mu, lv, kind)
            words = R.bits_of(out["shared"])
            for i, want in enumerate(expected):
                if want is not None:
                    assert words[i] == want, (D, i)
            assert np.isfinite(out["mu"]).all() and np.isfinite(out["lv"]).all() and np.isfinite(out["delta"]).all()
            # the fp32 evaluation agrees on the pairs whose mask is fixed by construction
            w32 = R.bits_of(R.mask_fp32(mu, lv))
            assert all(w32[i] == want for i, want in enumerate(expected) if want is not None)
        assert np.abs(lv[3] - lv[9]).max() == 40.0 and (lv[4, 0], lv[10, 0]) == (-20.0, 4.0)


# ---- 3. the library -----------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _nm(path, *flags):
    nm = shutil.which("nm") or shutil.which("llvm-nm", path="/opt/rocm/llvm/bin")
    assert nm, "no nm on this machine"
    return subprocess.run([nm] + list(flags) + [path], capture_output=True, text=True, check=True).stdout


def test_header_ctypes_table_and_exports_agree(monkeypatch):
    declared = sorted(set(re.findall(r"\b(dvae_weak_[a-zA-Z0-9_]+)\s*\(", _header())))
    assert declared == sorted(_weaklib.SIGNATURES)
    assert declared == sorted(["dvae_weak_version", "dvae_weak_last_error", "dvae_weak_aggregate_fwd", "dvae_weak_aggregate_bwd"])
    exported = sorted(set(re.findall(r" T (dvae_\w+)", _nm(os.path.abspath(_weaklib.LIB_PATH), "-D", "--defined-only"))))
    assert exported == declared
    kinds = {ctypes.c_void_p: "p", ctypes.c_int: "i", ctypes.c_long: "l", ctypes.c_double: "d"}
    for name, params in re.findall(r"\b(dvae_weak_[a-zA-Z0-9_]+)\s*\(([^)]*)\)", _header()):
        got = []
        for prm in [x.strip() for x in params.split(",") if x.strip() != "void"]:
            got.append("p" if "*" in prm else ("l" if prm.startswith("long") else ("d" if prm.startswith("double") else "i")))
        assert got == [kinds[t] for t in _weaklib.SIGNATURES[name]], name
    macros = {k: int(v) for k, v in re.findall(r"#define (DVAE_WEAK_\w+) (\d+)", _header())}
    mirrored = {"DVAE_WEAK_VERSION": _weaklib.VERSION, "DVAE_WEAK_MAX_D": _weaklib.MAX_D, "DVAE_WEAK_MAX_PAIRS": _weaklib.MAX_PAIRS,
                "DVAE_WEAK_GVAE": _weaklib.GVAE, "DVAE_WEAK_MLVAE": _weaklib.MLVAE, "DVAE_WEAK_THREADS": _weaklib.THREADS}
    assert macros == mirrored                                            # every macro of the header, none besides
    assert _weaklib.MAX_D == 64 and _weaklib.THREADS % 64 == 0 and _weaklib.KINDS == {"gvae": 0, "mlvae": 1}
    assert [_weaklib.group(D) for D in (1, 2, 3, 10, 16, 17, 33, 64)] == [1, 2, 4, 16, 16, 32, 64, 64]
    assert _weaklib.lib().dvae_weak_version() == _weaklib.VERSION == 1
    binding = open(_weaklib.__file__).read()
    assert 'Binding.for_library("weak", SIGNATURES, _RESTYPE' in binding and "LIB_PATH = _binding.path" in binding
    assert _weaklib._binding.last_error == "dvae_weak_last_error" and _weaklib._binding.signatures is _weaklib.SIGNATURES
    assert os.path.normpath(_weaklib.LIB_PATH).endswith(os.path.join("disentangling-vae_amd", "lib_scores", "libdvae_weak_hip.so"))
    monkeypatch.setenv("DVAE_WEAK_HIP_LIB", "/elsewhere/lib.so")             # the override, read when a binding is made
    assert _cabi.Binding.for_library("weak", {}, {}, "", subdir=os.path.join("..", "lib_scores")).path == "/elsewhere/lib.so"


def test_build_has_the_row_and_the_library_lies_in_lib_scores():
    build = _build()
    assert ("weak", ["weak_pairs"], "dvae_weak_hip.h") in [tuple(row) for row in build.SCORE_TARGETS]
    pkg = os.path.join(ROOT, "disentangling-vae_amd")
    assert os.path.abspath(build.WEAK_LIB) == os.path.join(pkg, "lib_scores", "libdvae_weak_hip.so") and os.path.exists(build.WEAK_LIB)
    assert "libdvae_weak_hip.so" in os.listdir(os.path.join(pkg, "lib_scores"))
    assert build.WEAK_SOURCES == ["weak_pairs"] and "weak_pairs" not in build.ALL_SOURCES
    others = {s for rows in (build.TARGETS, build.PLUGIN_TARGETS, build.SCORE_PLUGIN_TARGETS, build.EXTRA_TARGETS, build.MORE_TARGETS,
                             build.SCORE_TARGETS) for n, sources, _h in rows if n != "weak" for s in sources}
    assert "weak_pairs" not in others
    assert sorted(os.path.basename(h) for h in build.WEAK_HEADERS if "include" in h.split(os.sep)) == ["dvae_hip.h", "dvae_weak_hip.h"]
    text = open(os.path.join(pkg, "build.py")).read()
    row = [line for line in text.splitlines() if line.strip().startswith('("weak"')]
    assert len(row) == 1 and "TRAINING plugin" in row[0]                  # the row's comment says what it is
    # nothing of another library is linked in or included, and the training library does not know it
    src = open(os.path.join(CSRC, "weak_pairs.hip")).read()
    assert sorted(re.findall(r'^#include "([^"]+)"', src, re.M)) == ["../../include/dvae_weak_hip.h", "common.h", "last_error.h"]
    assert re.findall(r" U (dvae_\w+)", _nm(os.path.abspath(_weaklib.LIB_PATH), "-D")) == []
    assert "dvae_weak" not in _nm(os.path.abspath(_lib.LIB_PATH), "-D")


def test_source_obeys_the_rules_of_the_shared_plumbing():
    src = open(os.path.join(CSRC, "weak_pairs.hip")).read()
    assert len(re.findall(r'^#include "last_error\.h"', src, re.M)) == 1
    assert not re.search(r"\bthread_local\b", src) and not re.search(r"^void set_error\(", src, re.M)
    code = src.split("#include", 1)[1]
    assert not re.search(r"atomic", code)                                 # no atomics of any kind
    assert "while" not in code and "hipLaunchCooperativeKernel" not in code and "__shared__" not in code
    assert not re.search(r"hipMalloc|hipFree|hipMemcpy|hipMemset|Synchronize", code)   # the entry points only enqueue
    assert "double" not in code                                           # all arithmetic is fp32
    assert code.count("__shfl_xor") == 2 and "__ballot" in code           # the fixed tree over the lanes of a pair


def test_call_raises_with_the_librarys_own_error_text():
    h = _weaklib.lib()
    dummy = 1 << 20                                                # aligned non-NULL address, never dereferenced
    #      ml     pairs D  kind ml_agg shared delta stream
    fwd = [dummy, 5, 10, 0, dummy, dummy, None, None]
    #      ml     shared pairs D  kind dml   stream
    bwd = [dummy, dummy, 5, 10, 1, dummy, None]

    def put(good, i, v):
        return good[:i] + [v] + good[i + 1:]
    bad = [("dvae_weak_aggregate_fwd", put(fwd, i, None)) for i in (0, 4, 5)]
    bad += [("dvae_weak_aggregate_bwd", put(bwd, i, None)) for i in (0, 1, 5)]
    bad += [("dvae_weak_aggregate_fwd", put(fwd, 1, v)) for v in (0, -1, _weaklib.MAX_PAIRS + 1)]
    bad += [("dvae_weak_aggregate_bwd", put(bwd, 2, v)) for v in (0, -1, _weaklib.MAX_PAIRS + 1)]
    bad += [("dvae_weak_aggregate_fwd", put(fwd, 2, v)) for v in (0, -3, 65, 1000)]
    bad += [("dvae_weak_aggregate_bwd", put(bwd, 3, v)) for v in (0, -3, 65, 1000)]
    bad += [("dvae_weak_aggregate_fwd", put(fwd, 3, v)) for v in (-1, 2)] + [("dvae_weak_aggregate_bwd", put(bwd, 4, v)) for v in (-1, 2)]
    for name, args in bad:
        with pytest.raises(_lib.DvaeHipError) as e:
            _weaklib.call(name, *args)
        own = h.dvae_weak_last_error().decode()
        assert "invalid argument" in own and "weak_pairs.hip" in own, (name, args, own)
        assert str(e.value) == "%s failed (-1): %s" % (name, own)
    with pytest.raises(_lib.DvaeHipError, match="invalid argument.*DVAE_WEAK_MAX_D"):
        _weaklib.call("dvae_weak_aggregate_fwd", *put(fwd, 2, 65))
    assert "weak_pairs.hip" not in _dcilib.lib().dvae_dci_last_error().decode()        # every library keeps its own buffer


# ---- 4. the loss surface --------------------------------------------------------------------------------------------------------
HP = dict(rec_dist="bernoulli", reg_anneal=10000, betaH_B=4, betaB_initC=0, betaB_finC=25, betaB_G=1000, factor_G=6.4,
          latent_dim=10, lr_disc=1e-4, btcvae_A=1, btcvae_B=6.4, btcvae_G=1, n_data=1000)


def test_get_loss_f_keys_exports_and_defaults():
    assert L.WEAK_LOSSES == ["adagvae", "adamlvae"]
    assert L.LOSSES == ["VAE", "betaH", "betaB", "factor", "btcvae"] and L.DIP_LOSSES == ["dipI", "dipII"] and L.INFO_LOSSES == ["infovae"]
    for name, agg in (("adagvae", "gvae"), ("adamlvae", "mlvae")):
        f = L.get_loss_f(name, device="cpu", **HP)
        assert isinstance(f, L.WeakVaeLoss) and f.KIND == _lib.LOSS_BETAH and f.aggregation == agg and f.beta == 1
        assert f.steps_anneal == 10000 and f.rec_dist == "bernoulli"
        g = L.get_loss_f(name, device="cpu", weak_beta=4.0, **HP)
        assert g.beta == 4.0
        assert [k for k, _ in g.STORED] == ["recon_loss", "kl_loss", "shared_dims", "loss"]
        g.n_train_steps = 2500
        assert g._coefs(True) == dict(ANNEAL=0.25, BETA=4.0)             # BetaHLoss's: linear annealing of the KL term
        assert g._coefs(False) == dict(ANNEAL=1, BETA=4.0)
        assert f._replay_key.__func__ is L.WeakVaeLoss._replay_key        # the aggregation joins the replay key
    assert L.WeakVaeLoss._coefs is L.BetaHLoss._coefs
    with pytest.raises(ValueError):
        L.WeakVaeLoss(aggregation="labels")
    with pytest.raises(ValueError):
        L.get_loss_f("adavae", device="cpu", **HP)
    for name in ("WeakVaeLoss", "adaptive_group_posterior", "PairedFactorLoader", "draw_pair_partners"):
        assert name in disvae_amd.__all__, name
    assert disvae_amd.WeakVaeLoss is L.WeakVaeLoss and disvae_amd.adaptive_group_posterior is L.adaptive_group_posterior
    assert disvae_amd.PairedFactorLoader is DATA.PairedFactorLoader and disvae_amd.draw_pair_partners is DATA.draw_pair_partners


class _Comm:
    world_size, rank = 2, 0


def test_the_three_refusals_happen_before_any_device_work(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("device work before the refusal")
    monkeypatch.setattr(_weaklib, "lib", boom)
    monkeypatch.setattr(_weaklib, "call", boom)
    monkeypatch.setattr(_lib, "lib", boom)
    monkeypatch.setattr(L, "call", boom)

    class _Model:
        training = True

        def __init__(self, D):
            self.latent_dim = D

        @property
        def engine(self):
            boom()
    for name in L.WEAK_LOSSES:
        f = L.get_loss_f(name, device="cpu", **HP)
        with pytest.raises(ValueError, match="even number of rows"):
            f.fused_step(torch.zeros(5, 1, 32, 32), _Model(10), None, None)
        with pytest.raises(ValueError, match="latent_dim <= 64"):
            f.fused_step(torch.zeros(4, 1, 32, 32), _Model(65), None, None)
        f.comm = _Comm()
        with pytest.raises(NotImplementedError, match="data parallelism is not built"):
            f.fused_step(torch.zeros(4, 1, 32, 32), _Model(10), None, None)
        assert f.n_train_steps == 0
        # the reference signature cannot carry the aggregation: NOT a ValueError, which Trainer reads as "call call_optimize"
        with pytest.raises(NotImplementedError, match="fused_step.*adaptive_group_posterior") as e:
            f(torch.zeros(4, 1, 32, 32), torch.zeros(4, 1, 32, 32), (torch.zeros(4, 10), torch.zeros(4, 10)), True, None)
        assert not isinstance(e.value, ValueError)
    for mu, lv in ((torch.zeros(5, 10), torch.zeros(5, 10)), (torch.zeros(4, 65), torch.zeros(4, 65)), (torch.zeros(4, 3), torch.zeros(4, 4))):
        with pytest.raises(ValueError):
            L.adaptive_group_posterior(mu, lv, "gvae")
    with pytest.raises(ValueError):
        L.adaptive_group_posterior(torch.zeros(4, 3), torch.zeros(4, 3), "labels")
    w = torch.tensor([0, 1, 0b1011, -1, 1 << 62], dtype=torch.int64)
    assert L.popcount64(w).tolist() == [0, 1, 3, 64, 1]


# ---- 5. pairs -------------------------------------------------------------------------------------------------------------------
def _values(rows, sizes):
    strides = [int(np.prod(sizes[j + 1:])) for j in range(len(sizes))]
    return np.stack([(np.asarray(rows) // strides[j]) % sizes[j] for j in range(len(sizes))], axis=1)


@pytest.mark.parametrize("k", [1, 2, 3, 5, -1])
def test_draw_pair_partners(k):
    sizes = (1, 3, 2, 4)
    n_img, eligible = 24, 3
    g = torch.Generator().manual_seed(11)
    rows = torch.randint(0, n_img, (6000,), generator=g)
    partner, changed = DATA.draw_pair_partners(rows, sizes, k, g)
    assert partner.dtype == torch.int64 and changed.dtype == torch.int64 and partner.shape == changed.shape == rows.shape
    assert int(partner.min()) >= 0 and int(partner.max()) < n_img
    va, vb = _values(rows.numpy(), sizes), _values(partner.numpy(), sizes)
    differs = va != vb
    bits = np.stack([(changed.numpy() >> j) & 1 for j in range(len(sizes))], axis=1).astype(bool)
    assert np.array_equal(differs, bits)                                  # the partner differs in exactly the changed factors
    assert not bits[:, 0].any()                                           # a factor with one value is never changed
    count = bits.sum(axis=1)
    if k == -1:
        assert set(count.tolist()) == {1, 2}                              # 1 .. eligible - 1: one factor always stays shared
        assert abs((count == 1).mean() - 0.5) < 0.03
    else:
        assert (count == min(k, eligible)).all()
    # every eligible factor is reached, and from every value every OTHER value
    for j in (1, 2, 3):
        assert bits[:, j].any()
        seen = {(int(a), int(b)) for a, b in zip(va[bits[:, j], j], vb[bits[:, j], j])}
        assert seen == {(a, b) for a in range(sizes[j]) for b in range(sizes[j]) if a != b}, (j, seen)
    if k == 1:                                                             # uniform over the eligible factors
        share = bits[:, 1:].mean(axis=0)
        assert np.abs(share - 1 / 3).max() < 0.03
    # the same seed gives the same output; the global generator is not touched
    state = torch.get_rng_state()
    g2 = torch.Generator().manual_seed(11)
    rows2 = torch.randint(0, n_img, (6000,), generator=g2)
    again = DATA.draw_pair_partners(rows2, sizes, k, g2)
    assert torch.equal(again[0], partner) and torch.equal(again[1], changed) and torch.equal(torch.get_rng_state(), state)


def test_draw_pair_partners_refusals_and_one_eligible_factor():
    g = torch.Generator().manual_seed(0)
    rows = torch.arange(5)
    for k in (1, 4, -1):                                                   # one eligible factor: it is the one that changes
        partner, changed = DATA.draw_pair_partners(rows, (1, 5, 1), k, g)
        assert (partner != rows).all() and (changed == 2).all()
    with pytest.raises(ValueError):
        DATA.draw_pair_partners(rows, (1, 1), 1, g)
    for k in (0, -2):
        with pytest.raises(ValueError):
            DATA.draw_pair_partners(rows, (1, 5, 1), k, g)


def test_paired_factor_loader_on_the_cpu():
    sizes = (3, 4, 2)
    n = 24
    images = torch.arange(n, dtype=torch.uint8).view(n, 1, 1, 1).expand(n, 1, 4, 4).contiguous()     # an image holds its row number
    loader = DATA.PairedFactorLoader(images, sizes, batch_size=5, k=1, device="cpu")
    assert len(loader) == 5 and len(loader.dataset) == n
    torch.manual_seed(3)
    batches = list(loader)
    assert [b.shape[0] for b, _ in batches] == [10, 10, 10, 10, 8] and all(b.dtype == torch.uint8 and b.shape[1:] == (1, 4, 4) for b, _ in batches)
    assert [c.shape[0] for _, c in batches] == [5, 5, 5, 5, 4]
    first = torch.cat([b[:b.shape[0] // 2, 0, 0, 0] for b, _ in batches]).long()
    second = torch.cat([b[b.shape[0] // 2:, 0, 0, 0] for b, _ in batches]).long()
    changed = torch.cat([c for _, c in batches])
    # the first members are the reference loader's epoch order, the partners one more draw of the global generator behind it
    torch.manual_seed(3)
    order = DATA.DeviceImageLoader.epoch_order(n)
    g = torch.Generator().manual_seed(int(torch.empty((), dtype=torch.int64).random_().item()))
    partner, want_changed = DATA.draw_pair_partners(order, sizes, 1, g)
    assert torch.equal(first, order) and sorted(first.tolist()) == list(range(n))
    assert torch.equal(second, partner) and torch.equal(changed, want_changed)
    state = torch.get_rng_state()
    torch.manual_seed(3)
    list(loader)
    assert torch.equal(torch.get_rng_state(), state)                      # an epoch consumes three draws, whatever it yields
    va, vb = _values(first.numpy(), sizes), _values(second.numpy(), sizes)
    assert ((va != vb).sum(axis=1) == 1).all()
    second_epoch = torch.cat([b[b.shape[0] // 2:, 0, 0, 0] for b, _ in loader]).long()
    assert not torch.equal(second_epoch, second)                          # a new epoch draws new pairs
    with pytest.raises(ValueError, match="enumerate 24 images"):
        DATA.PairedFactorLoader(images[:23], sizes, device="cpu")
    with pytest.raises(ValueError):
        DATA.PairedFactorLoader(images, sizes, k=0, device="cpu")
    assert len(DATA.PairedFactorLoader(images, sizes, batch_size=4, device="cpu")) == 6
    assert len(DATA.PairedFactorLoader(images, sizes, batch_size=64, device="cpu")) == 1
