"""CPU: the host side of the per-image scores (disvae_amd/likelihood.py, Evaluator.compute_log_likelihood) -- argument errors
raised before any device work, the decoder-pass planner, and the new C-ABI exports (header, ctypes table, plan ops)."""
import ctypes
import os
import re

import pytest
import torch

import disvae_amd
from disvae_amd import _lib, Evaluator, log_likelihood, per_image_losses
from disvae_amd import likelihood as LL
from disvae_amd.models.losses import get_loss_f
from disvae_amd.models.vae import init_specific_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dvae_recon_rows", "dvae_recon_rows_ws_floats", "dvae_iw_loglik")
HP = dict(rec_dist="bernoulli", reg_anneal=0, betaH_B=4, betaB_initC=0, betaB_finC=25, betaB_G=1000, factor_G=6.4,
          latent_dim=4, lr_disc=1e-4, btcvae_A=1, btcvae_B=6.4, btcvae_G=1)


def test_exported_from_the_package():
    assert disvae_amd.log_likelihood is LL.log_likelihood and disvae_amd.per_image_losses is LL.per_image_losses
    assert {"log_likelihood", "per_image_losses"} <= set(disvae_amd.__all__)


def test_argument_errors():
    model = init_specific_model("Burgess", (1, 32, 32), 4)             # on the CPU
    x = torch.rand(3, 1, 32, 32)
    for bad in (0, -1):
        with pytest.raises(ValueError, match="n_samples"):
            log_likelihood(model, x, n_samples=bad)
    with pytest.raises(ValueError, match="Unkown distribution"):
        log_likelihood(model, x, n_samples=4, rec_dist="poisson")
    with pytest.raises(ValueError, match="Unkown distribution"):
        per_image_losses(model, x, rec_dist="poisson")
    with pytest.raises(_lib.DvaeHipError, match="no CPU fallback"):
        log_likelihood(model, x, n_samples=4)
    with pytest.raises(_lib.DvaeHipError, match="no CPU fallback"):
        per_image_losses(model, x)
    assert model.training                                                # nothing ran: the mode is as it was


def test_evaluator_argument_errors():
    model = init_specific_model("Burgess", (1, 32, 32), 4)
    ev = Evaluator(model, get_loss_f("VAE", **HP), device=torch.device("cpu"), is_progress_bar=False)
    loader = [(torch.rand(2, 1, 32, 32), None)]
    with pytest.raises(ValueError, match="n_samples"):
        ev.compute_log_likelihood(loader, n_samples=0)
    with pytest.raises(_lib.DvaeHipError):
        ev.compute_log_likelihood(loader, n_samples=2)
    ev.loss_f.rec_dist = "poisson"
    with pytest.raises(ValueError, match="Unkown distribution"):
        ev.compute_log_likelihood(loader, n_samples=2)


def _covers(plan, n_img, K):
    """Every (image, sample) exactly once, the samples of an image in order, first / last pass of an image well defined."""
    seen = {}
    for i0, i1, k0, k1 in plan:
        assert 0 <= i0 < i1 <= n_img and 0 <= k0 < k1 <= K
        for i in range(i0, i1):
            assert seen.get(i, 0) == k0, (i, k0)
            seen[i] = k1
    assert seen == {i: K for i in range(n_img)}


@pytest.mark.parametrize("n_img,K,R", [(37, 64, 256), (5, 1, 256), (300, 1, 256), (3, 256, 256), (7, 255, 256), (37, 17, 256),
                                       (4, 300, 256), (2, 1000, 256), (1, 513, 256), (3, 7, 8)])
def test_pass_planner(n_img, K, R):
    plan = LL.plan_passes(n_img, K, R)
    _covers(plan, n_img, K)
    assert all((i1 - i0) * (k1 - k0) <= R for i0, i1, k0, k1 in plan)
    if K <= R:
        per = max(1, R // K)                                             # images per pass
        assert all(k0 == 0 and k1 == K for _, _, k0, k1 in plan)
        assert [i1 - i0 for i0, i1, _, _ in plan] == [per] * (n_img // per) + ([n_img % per] if n_img % per else [])
    else:                                                                # K > R: one image spans ceil(K / R) passes
        assert all(i1 - i0 == 1 for i0, i1, _, _ in plan)
        assert len(plan) == n_img * (-(-K // R))
        assert [k1 - k0 for i0, _, k0, k1 in plan if i0 == 0] == [R] * (K // R) + ([K % R] if K % R else [])


def test_pass_planner_at_the_private_row_budget():
    R = LL._ScorePasses.MAX_ROWS
    assert LL.plan_passes(37, 64, R)[0] == (0, R // 64, 0, 64)
    assert len(LL.plan_passes(1, 300, R)) == 2                            # the K = 300 of the GPU tests spans two passes


def _declared():
    txt = open(os.path.join(ROOT, "include", "dvae_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(dvae_[a-zA-Z0-9_]+)\s*\(", txt))


def test_new_symbols_in_header_ctypes_and_plan_ops():
    assert set(NEW) <= _declared()
    assert set(NEW) <= set(_lib.SIGNATURES)
    h = _lib.lib()
    for name in NEW:
        assert h.dvae_plan_op(name.encode()) >= 0, name
    assert h.dvae_version() == 109


def test_argument_checks_before_any_launch():
    """NULL pointers, K < 1, a row length that is not a multiple of 4, an unknown distribution: refused without a launch."""
    h = _lib.lib()
    dummy = 1 << 20                                                       # aligned non-NULL address, never dereferenced
    bad = [("dvae_recon_rows", (None, dummy, 0, 1, 1, 16, 0, None, dummy, None)),
           ("dvae_recon_rows", (dummy, dummy, 0, 1, 0, 16, 0, None, dummy, None)),
           ("dvae_recon_rows", (dummy, dummy, 0, 1, 1, 18, 0, None, dummy, None)),
           ("dvae_recon_rows", (dummy, dummy, 0, 1, 1, 16, 7, None, dummy, None)),
           ("dvae_recon_rows", (dummy + 4, dummy, 0, 1, 1, 16, 0, None, dummy, None)),
           ("dvae_recon_rows_ws_floats", (1, 1, 16, None)),
           ("dvae_recon_rows_ws_floats", (1, 1, 18, dummy)),
           ("dvae_iw_loglik", (dummy, dummy, None, None, None, 1, 1, 4, 1, 1, 1, None, None, None, None)),
           ("dvae_iw_loglik", (dummy, dummy, None, dummy, dummy, 1, 1, 4, 1, 1, 1, dummy, dummy, None, None)),
           ("dvae_iw_loglik", (dummy, dummy, dummy, dummy, dummy, 1, 4, 4, 2, 1, 1, dummy, dummy, None, None)),
           ("dvae_iw_loglik", (dummy, dummy, dummy, dummy, dummy, 1, 2, 4, 2, 1, 1, dummy, None, None, None))]
    for name, args in bad:
        with pytest.raises(_lib.DvaeHipError, match="invalid argument"):
            _lib.call(name, *args)
        # the same through the plan trampoline
        arr = (_lib.PlanEntry * 1)()
        arr[0].op, arr[0].nargs = h.dvae_plan_op(name.encode()), len(args)
        for i, (t, a) in enumerate(zip(_lib.SIGNATURES[name], args)):
            arr[0].args[i] = _lib._pack(t, a)
        assert h.dvae_plan_run(ctypes.addressof(arr), 1) != 0 and b"invalid argument" in h.dvae_last_error()


def test_recon_rows_workspace_size():
    """Per-slice sums of rows longer than one 1024-element column slice: n_img * K * slices floats; none otherwise.  A row
    length that needs a workspace is refused without one (before any launch)."""
    def ws(n, K, row):
        v = ctypes.c_long(-1)
        _lib.call("dvae_recon_rows_ws_floats", n, K, row, ctypes.addressof(v))
        return v.value
    assert ws(3, 5, 1024) == 0 and ws(3, 5, 16) == 0
    assert ws(3, 5, 1028) == 3 * 5 * 2 and ws(2, 128, 12288) == 2 * 128 * 12 and ws(7, 1, 4096) == 7 * 4
    dummy = 1 << 20
    with pytest.raises(_lib.DvaeHipError, match="workspace"):
        _lib.call("dvae_recon_rows", dummy, dummy, 0, 1, 1, 2048, 0, None, dummy, None)
