"""-m gpu: the data-set level ELBO decomposition (libdvae_eval_hip.so, csrc/elbo_decomp.hip; Evaluator.compute_elbo_decomposition)
against the fp64 restatement of tests/decomp_ref.py -- kernel parity on both sides of every dispatch switch (padded widths 4 / 8 /
12 / 16, the run-time-D kernel with z in LDS and re-read, one chunk / several), the degenerate sample, the memory contract of
both launching entry points, and the Evaluator end to end.

Tolerances (tests/test_gpu_metrics.py's for the entropy estimator): per-sample log q(z_s) rtol 2e-6 + atol 2e-6, entropies and
means rtol 1e-5; mi / tc / dw_kl / kl are differences of those, held to decomp_ref.derived_atol."""
import functools
import json
import logging
import math

import numpy as np
import pytest
import torch

import decomp_ref as R
from gpu_util import DEV, dev, stream
from guard_util import Guarded, run_contract
from disvae_amd import _evallib, _lib, Evaluator
from disvae_amd.models.losses import get_loss_f
from disvae_amd.models.vae import init_specific_model

pytestmark = pytest.mark.gpu
L = _evallib.JOINT_CHUNK
HP = dict(rec_dist="bernoulli", reg_anneal=10000, betaH_B=4, betaB_initC=0, betaB_finC=25,
          betaB_G=1000, factor_G=6.4, latent_dim=10, lr_disc=1e-4, btcvae_A=1, btcvae_B=6.4, btcvae_G=1)

# (N, D, S).  D: 1, 3 -> width 4; 10 -> 12; 16 -> 16; 17, 33 -> run-time D with z in LDS.
# N <= L: one chunk; N = L + 1, 2049 (S <= 256: one sample block): two chunks; S = 257: a second, ragged sample block.
SHAPES = [(1, 1, 1), (7, 3, 5), (8, 10, 256), (9, 10, 257), (1000, 10, 300), (2049, 16, 257), (1500, 17, 100), (300, 33, 70),
          (L - 1, 10, 64), (L, 10, 64), (L + 1, 10, 64)]
# two more dispatch paths the shapes above do not reach: D = 7 -> width 8 (three chunks), D = 50 -> run-time D with z re-read
# from memory.  They are about the path, not about numerical stress: the broad family only.
PATH_SHAPES = [(5000, 7, 130), (40, 50, 9)]
FAMILIES = {"broad": (-2.0, 0.5), "sharp": (-10.0, 1.0)}
CASES = [(N, D, S, f) for f in sorted(FAMILIES) for N, D, S in SHAPES] + [(N, D, S, "broad") for N, D, S in PATH_SHAPES]
# Per-sample log q(z_s) bound, as a multiple of rtol 2e-6 + atol 2e-6, where a case was measured to miss it (the
# kernel's and the fp32-torch restatement's worst error against fp64, the bound at most twice the larger):
#   (300, 33, 70) sharp: kernel 1.093 (max abs 1.02e-5 on a sample with |log q| = 3.7), fp32 torch 0.17.  D = 33 with logvar
#   down to -10: c_n and the quadratic form are sequential fp32 sums of 33 terms of magnitude ~50 (half an ulp = 1.9e-6 each).
LOGQZ_BOUND = {(300, 33, 70, "sharp"): 2.0}


@functools.lru_cache(maxsize=None)
def problem(N, D, S, family):
    """Inputs (fp32, CPU) and their fp64 decomposition: computed once, shared by the tests, never modified."""
    mean, logvar, rows, eps = R.clustered_posteriors(N, D, S, seed=1000 * D + N % 997, logvar_range=FAMILIES[family])
    z = R.sample_z(mean, logvar, rows, eps)                       # fp32: the samples both sides are given
    assert z.shape == eps.shape == (S, D) and rows.shape == (S,) and 0 <= int(rows.min()) and int(rows.max()) < N
    return mean, logvar, rows, eps, z, R.decomposition(z, eps, rows, mean, logvar)


def run_kernels(mean, logvar, rows, eps, z, poison_ws=True):
    """Both entry points of the new library + dvae_latent_entropy on the [D, S] image -> the decomposition's pieces."""
    (N, D), S = mean.shape, z.shape[0]
    assert z.shape == eps.shape == (S, D) and logvar.shape == (N, D) and rows.shape == (S,)    # the kernels trust these sizes
    assert rows.dtype == torch.int64 and 0 <= int(rows.min()) and int(rows.max()) < N
    E = _evallib.lib()
    need = E.dvae_eval_joint_logq_ws_floats(N, D, S)
    ws = torch.full((need,), float("nan"), device=DEV) if poison_ws else torch.empty(need, device=DEV)
    logqz, H = torch.empty(S, device=DEV), torch.empty(1, device=DEV)
    zd, md, ld, ed, rd = dev(z), dev(mean), dev(logvar), dev(eps), rows.to(DEV)
    _evallib.call("dvae_eval_joint_logq", zd.data_ptr(), md.data_ptr(), ld.data_ptr(), N, D, S, ws.data_ptr(), logqz.data_ptr(),
                  H.data_ptr(), stream())
    qc, pz, means = torch.empty(S, device=DEV), torch.empty(S, device=DEV), torch.empty(2, device=DEV)
    _evallib.call("dvae_eval_sample_terms", zd.data_ptr(), ed.data_ptr(), ld.data_ptr(), rd.data_ptr(), N, D, S, qc.data_ptr(),
                  pz.data_ptr(), means.data_ptr(), stream())
    ws2 = torch.empty(_lib.lib().dvae_latent_entropy_ws_floats(N, D, S), device=DEV)
    Hd = torch.empty(D, device=DEV)
    z_ds = zd.t().contiguous()
    _lib.call("dvae_latent_entropy", z_ds.data_ptr(), md.data_ptr(), ld.data_ptr(), N, D, S, ws2.data_ptr(), Hd.data_ptr(), stream())
    torch.cuda.synchronize()
    return {"logqz": logqz.cpu().double(), "logqz_condx": qc.cpu().double(), "logpz": pz.cpu().double(),
            "H_z": H.item(), "H_zCx": -means[0].item(), "mean_logpz": means[1].item(), "H_z_d": [float(v) for v in Hd.cpu().double()]}


def assert_decomposition(got, ref, what):
    """got: H_z, H_z_d, H_zCx and (mean_logpz or the derived terms) in fp32 precision; ref: decomp_ref.decomposition."""
    for k in ("H_z", "H_zCx"):
        print("%s %s: got %.9g ref %.9g rel %.2e" % (what, k, got[k], ref[k], abs(got[k] - ref[k]) / abs(ref[k])))
        np.testing.assert_allclose(got[k], ref[k], rtol=1e-5, err_msg=what + " " + k)
    np.testing.assert_allclose(got["H_z_d"], ref["H_z_d"], rtol=1e-5, err_msg=what + " H_z_d")
    if "mean_logpz" in got:
        np.testing.assert_allclose(got["mean_logpz"], ref["mean_logpz"], rtol=1e-5, err_msg=what + " mean logpz")
        mi = got["H_z"] - got["H_zCx"]
        tc = math.fsum(got["H_z_d"]) - got["H_z"]
        dw = -math.fsum(got["H_z_d"]) - got["mean_logpz"]
        got = dict(got, mi=mi, tc=tc, dw_kl=dw, kl=mi + tc + dw)
    atol = R.derived_atol(ref)
    for k in ("mi", "tc", "dw_kl", "kl"):
        print("%s %s: got %.9g ref %.9g err/atol %.3f" % (what, k, got[k], ref[k], abs(got[k] - ref[k]) / atol))
        assert abs(got[k] - ref[k]) <= atol, (what, k, got[k], ref[k], atol)


# ---- 1. kernel parity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,S,family", CASES)
def test_kernels_vs_fp64(N, D, S, family):
    mean, logvar, rows, eps, z, ref = problem(N, D, S, family)
    if family == "broad" and N >= 1000:
        # many data points contribute to each logsumexp (an estimate saturated at log N exercises the self term only)
        assert ref["mi"] < 0.9 * math.log(N), (ref["mi"], math.log(N))
    got = run_kernels(mean, logvar, rows, eps, z)
    what = "N%d D%d S%d %s" % (N, D, S, family)
    worst = {}
    for k in ("logqz", "logqz_condx", "logpz"):
        err = (got[k] - ref[k]).abs()
        tol = 2e-6 * ref[k].abs() + 2e-6
        worst[k] = (err / tol).max().item()
        print("%s %s: worst err / tol %.3f (max abs err %.3e)" % (what, k, worst[k], err.max().item()))
        assert torch.isfinite(got[k]).all(), (what, k)
    assert worst["logqz"] <= LOGQZ_BOUND.get((N, D, S, family), 1.0), (what, worst)
    assert worst["logqz_condx"] <= 1.0 and worst["logpz"] <= 1.0, (what, worst)
    assert_decomposition(got, ref, what)


def test_sample_without_any_finite_density_is_minus_inf_not_nan():
    """(z - mu)^2 overflows fp32 for every data point: each density is -inf, log q(z_s) = -inf (as torch.logsumexp gives), never
    NaN, and the other samples of the workgroup and chunk are what they are without it."""
    N, D, S = L + 1, 10, 70
    mean, logvar, rows, eps, z, ref = problem(N, D, S, "broad")
    z = z.clone()
    z[33, 4] = 1e25
    got = run_kernels(mean, logvar, rows, eps, z)
    plain = run_kernels(mean, logvar, rows, eps, problem(N, D, S, "broad")[4])
    lq = got["logqz"]
    assert lq[33] == -math.inf and not torch.isnan(lq).any()
    keep = torch.arange(S) != 33
    assert torch.equal(lq[keep], plain["logqz"][keep])                       # bit for bit
    assert got["H_z"] == math.inf
    assert got["logpz"][33] == -math.inf and not torch.isnan(got["logpz"]).any() and not torch.isnan(got["logqz_condx"]).any()
    assert torch.equal(got["logqz_condx"], plain["logqz_condx"])
    # the same sample with ONE finite density, at the last data point -- whose chunk ends in padding records (N = L + 1 is no
    # multiple of 8): a padding record must count as density -inf for this z too (its exp(-logvar) = 0 times an infinite
    # square would be NaN), so the result is that one density - log N
    mean2 = mean.clone()
    mean2[N - 1, 4] = 1e25
    got2 = run_kernels(mean2, logvar, rows, eps, z)
    ref33 = R.aggregate_logq(z[33:34], mean2, logvar)[0].item()
    assert math.isfinite(ref33) and not torch.isnan(got2["logqz"]).any()
    assert abs(got2["logqz"][33].item() - ref33) <= 2e-6 * abs(ref33) + 2e-6, (got2["logqz"][33].item(), ref33)


# ---- 2. memory contract --------------------------------------------------------------------------------------------------------
CONTRACT_SHAPES = [(9, 10, 257), (300, 33, 70), (L + 1, 10, 64)]


def _eval_call(name):
    def fn(args):
        _evallib.call(name, *[a.ptr if isinstance(a, Guarded) else a for a in args])
    return fn


@pytest.mark.parametrize("N,D,S", CONTRACT_SHAPES)
def test_memory_contract_joint_logq(N, D, S):
    """Guards untouched, inputs unchanged, every output element written, bits equal to the run on plain tensors whatever the
    workspace and the surroundings hold (NaN at 256-byte alignment; -1e30 at the weakest alignment promised: the element's own)."""
    mean, logvar, rows, eps, z, _ = problem(N, D, S, "broad")
    nws = _evallib.lib().dvae_eval_joint_logq_ws_floats(N, D, S)

    def build(al):
        return [al.inp("z", z, align=4), al.inp("mean", mean, align=4), al.inp("logvar", logvar, align=4), N, D, S,
                al.ws("ws", (nws,), align=4), al.out("logqz", (S,), align=4), al.out("H_joint", (1,), align=4), stream()]
    run_contract("dvae_eval_joint_logq", build, fn=_eval_call("dvae_eval_joint_logq"))


@pytest.mark.parametrize("N,D,S", CONTRACT_SHAPES)
def test_memory_contract_sample_terms(N, D, S):
    mean, logvar, rows, eps, z, _ = problem(N, D, S, "broad")

    def build(al):
        return [al.inp("z", z, align=4), al.inp("eps", eps, align=4), al.inp("logvar", logvar, align=4),
                al.inp("rows", rows, align=8), N, D, S, al.out("logqz_condx", (S,), align=4), al.out("logpz", (S,), align=4),
                al.out("means", (2,), align=4), stream()]
    run_contract("dvae_eval_sample_terms", build, fn=_eval_call("dvae_eval_sample_terms"))


# ---- 3. Evaluator end to end ---------------------------------------------------------------------------------------------------
def _setup(tmp_path, seed=5):
    img, D, N, S = (1, 32, 32), 10, 96, 64
    torch.manual_seed(seed)
    model = init_specific_model("Burgess", img, D).to(DEV).train()
    gen = torch.Generator().manual_seed(seed + 1)
    x = torch.rand((N,) + img, generator=gen)
    loader = [(x[i:i + 32], None) for i in range(0, N, 32)]
    ev = Evaluator(model, get_loss_f("VAE", device=torch.device(DEV), **HP), device=torch.device(DEV),
                   logger=logging.getLogger("decomp"), save_dir=str(tmp_path), is_progress_bar=False)
    rows = torch.randperm(N, generator=gen)[:S]
    eps = torch.randn(S, D, generator=gen)
    return model, ev, loader, x, rows, eps


def test_evaluator_vs_fp64_restatement(tmp_path):
    model, ev, loader, x, rows, eps = _setup(tmp_path)
    got = ev.compute_elbo_decomposition(loader, sample_idx=rows, eps=eps)
    assert model.training                                                     # mode restored
    model.eval()
    with torch.no_grad():
        mean, logvar = model.encoder(x.to(DEV))
    model.train()
    ref = R.decomposition(R.sample_z(mean.cpu().double(), logvar.cpu().double(), rows, eps.double()), eps, rows, mean.cpu(),
                          logvar.cpu())
    assert got["n_samples"] == 64 and got["n_data"] == 96 and len(got["H_z_d"]) == 10
    assert set(got) == {"H_z", "H_z_d", "H_zCx", "mi", "tc", "dw_kl", "kl", "n_samples", "n_data"}
    assert got["kl"] == got["mi"] + got["tc"] + got["dw_kl"]
    assert_decomposition(got, ref, "evaluator")
    # H_z_d is dvae_latent_entropy itself, on the [D, S] image of the same samples
    z = (mean.index_select(0, rows.to(DEV)) + torch.exp(0.5 * logvar.index_select(0, rows.to(DEV))) * eps.to(DEV)).contiguous()
    z_ds = z.t().contiguous()
    ws = torch.empty(_lib.lib().dvae_latent_entropy_ws_floats(96, 10, 64), device=DEV)
    H = torch.empty(10, device=DEV)
    _lib.call("dvae_latent_entropy", z_ds.data_ptr(), mean.data_ptr(), logvar.data_ptr(), 96, 10, 64, ws.data_ptr(), H.data_ptr(),
              stream())
    assert got["H_z_d"] == [float(v) for v in H.cpu().double()]


def test_evaluator_seeds_random_states_whole_data_set_and_log_file(tmp_path):
    model, ev, loader, x, rows, eps = _setup(tmp_path, seed=9)
    cpu0, dev0 = torch.get_rng_state(), torch.cuda.get_rng_state()
    a = ev.compute_elbo_decomposition(loader, n_samples=64, seed=3)
    b = ev.compute_elbo_decomposition(loader, n_samples=64, seed=3)
    c = ev.compute_elbo_decomposition(loader, n_samples=64, seed=4)
    assert a == b and a != c and all(math.isfinite(a[k]) for k in ("H_z", "H_zCx", "mi", "tc", "dw_kl", "kl"))
    assert torch.equal(torch.get_rng_state(), cpu0) and torch.equal(torch.cuda.get_rng_state(), dev0)
    assert model.training
    # n_samples=None: every image once, in data-set order
    noise = torch.randn(96, 10, generator=torch.Generator().manual_seed(2))
    full = ev.compute_elbo_decomposition(loader, n_samples=None, eps=noise)
    assert full["n_samples"] == full["n_data"] == 96
    assert full == ev.compute_elbo_decomposition(loader, sample_idx=torch.arange(96), eps=noise)
    assert full != ev.compute_elbo_decomposition(loader, sample_idx=torch.arange(95, -1, -1), eps=noise)
    with pytest.raises(ValueError, match="exceeds"):
        ev.compute_elbo_decomposition(loader, n_samples=97)
    # Evaluator.__call__: the file only on request, the return value the reference's
    ev(loader, is_losses=False)
    assert not (tmp_path / "elbo_decomposition.log").exists()
    assert ev(loader, is_losses=False, is_decomposition=True, n_samples_decomposition=64) == (None, None)
    assert json.load(open(tmp_path / "elbo_decomposition.log")) == ev.compute_elbo_decomposition(loader, n_samples=64)
    assert model.training
    assert _lib.lib().dvae_version() == 109
