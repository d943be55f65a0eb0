"""-m gpu: the whole training step on poisoned buffers.

The engine allocates every activation, gradient, weight-image and workspace buffer with torch.empty and caches them per batch
size, so production depends on no kernel ever reading memory that this step has not written first -- a split-K partial of a
workgroup that had no work, a padding column, the tail rows of a buffer after a batch-size switch.  What such a read finds is
what the same-shaped step before left there: very often the right value.  Here twin models run the same five steps (batch sizes
16, 16, 7, 16, 7: buffers are cached per batch size, plans are keyed on addresses) from the same seed on the same injected data
and noise; before every step one twin fills every such buffer with NaN, in place.  Losses of every step, the parameters and the
gradients after the last step must be bit-identical.

Poisoned (found by walking the attributes of the engine, the loss object's scratch and the discriminator -- a buffer added later
is poisoned too): everything allocated with torch.empty -- the _Buffers of EVERY cached batch size, _Images.buf, the three
weight-gradient workspaces, the scratch's latent buffers, the discriminator's activations and workspaces -- and every
parameter's slice of the gradient arenas.

Left alone, with the reason:
  * parameters (arena.flat), Adam state, the step counters: state carried from step to step by design;
  * scratch.coef (the coefficient vector: written by the host side of each step, read by every loss kernel), scratch.log_w
    (constants of the data set, written once by the host);
  * scratch.scal, packed, partials, kl_dim, disc_sums: allocated with torch.zeros (models/losses.py, _Scratch) -- slots the
    kernels of a given loss do not define are read back by the host's logging as zeros;
  * the padding between the parameters' slices of the gradient arena (torch.zeros; all-reduced as one flat buffer when sharded);
  * the loss object's _static input copies and the batch itself: inputs of the step, not its workspace.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from disvae_amd import _lib
from disvae_amd.data import DeviceImageLoader
from disvae_amd.models.losses import get_loss_f
from disvae_amd.models.vae import init_specific_model

DEV = "cuda"
HP = dict(rec_dist="bernoulli", reg_anneal=10000, betaH_B=4, betaB_initC=0, betaB_finC=25, betaB_G=1000, factor_G=6.4,
          lr_disc=1e-4, btcvae_A=1, btcvae_B=6.4, btcvae_G=1)
BATCHES = (16, 16, 7, 16, 7)
ZEROS_OR_STATE = {"coef", "log_w", "scal", "packed", "partials", "kl_dim", "disc_sums"}     # of _Scratch: see the module docstring
INT_POISON = 0x5A5A5A5A


def _walk(obj, path, seen, skip=()):
    """(path, tensor) for every device tensor reachable through attributes, lists, tuples and dicts of the project's objects."""
    if isinstance(obj, torch.Tensor):
        if obj.is_cuda and not isinstance(obj, torch.nn.Parameter):
            yield path, obj
    elif isinstance(obj, dict):
        for k, v in obj.items():
            yield from _walk(v, "%s[%r]" % (path, k), seen, skip)
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            yield from _walk(v, "%s[%d]" % (path, i), seen, skip)
    elif (type(obj).__module__ or "").startswith("disvae_amd") and hasattr(obj, "__dict__") and id(obj) not in seen \
            and not isinstance(obj, (ctypes.Structure, ctypes.Array, ctypes._SimpleCData)):
        seen.add(id(obj))
        for k, v in vars(obj).items():
            if k in skip or k in ("_parameters", "_buffers", "_modules"):
                continue
            yield from _walk(v, path + "." + k, seen, skip)


def _workspace_tensors(model, loss_f):
    seen = set()
    found = list(_walk(model.engine, "engine", seen, skip=("arena",)))
    sc = loss_f._scratch
    if sc is not None:
        found += [(p, t) for p, t in _walk(sc, "scratch", seen) if p.split(".")[1].split("[")[0] not in ZEROS_OR_STATE]
    disc = getattr(loss_f, "discriminator", None)
    if disc is not None:
        found += list(_walk(disc, "discriminator", seen, skip=("_arena", "_grad_views")))
    return found


def _poison(model, loss_f):
    torch.cuda.synchronize()
    found = _workspace_tensors(model, loss_f)
    for _, t in found:
        t.fill_(float("nan")) if t.dtype.is_floating_point else t.fill_(INT_POISON if t.dtype != torch.uint8 else 0x5A)
    arenas = [model.arena] + ([loss_f.discriminator.arena] if hasattr(loss_f, "discriminator") else [])
    for ar in arenas:
        for name in ar.shapes:
            ar.view(name, grad=True).fill_(float("nan"))
    torch.cuda.synchronize()
    return [p for p, _ in found]


def _check_walk(paths, model, loss_f, batch_sizes, loss):
    """The walk found at least the buffers the module docstring names."""
    joined = "\n".join(paths)
    for need in ("engine._ws", "engine._ws_side", "engine._ws_wg2", "engine._images.buf"):
        assert any(p == need for p in paths), (need, joined)
    for B in batch_sizes:
        for attr in ("a_flat", "lat3", "recon", "g_logit", "gd3", "dz", "enc_act[0]", "dec_gact[0]"):
            assert "engine._bufs[%d].%s" % (B, attr) in paths, (B, attr, joined)
    if loss == "btcvae":
        assert any(p.startswith("scratch.lat[('rowstats'") for p in paths) and any(p.startswith("scratch.lat[('tc_tmp'") for p in paths)
    if loss == "factor":
        assert any(p.startswith("scratch.lat[('disc_in'") for p in paths) and any(p.startswith("discriminator._acts[") for p in paths)


def _make(loss, img, D, seed=33):
    torch.manual_seed(seed)
    model = init_specific_model("Burgess", img, D)
    opt = torch.optim.Adam(model.parameters(), lr=5e-4)
    loss_f = get_loss_f(loss, n_data=202599, device=torch.device(DEV), latent_dim=D, **HP)
    model.to(DEV)
    model.train()
    return model, opt, loss_f


def _run(loss, img, D, replay, poisoned, batches, u8=False):
    model, opt, loss_f = _make(loss, img, D)
    loss_f.replay = replay
    gen = torch.Generator().manual_seed(8)
    if u8:
        n = sum(batches[:3])
        loader = DeviceImageLoader(torch.randint(0, 256, (n,) + img, dtype=torch.uint8, generator=gen).to(DEV),
                                   batch_size=batches[0], shuffle=False)
        feed = []
        while len(feed) < len(batches):
            feed += [b for b, _ in loader]
        feed = feed[:len(batches)]
        assert [b.shape[0] for b in feed] == list(batches) and feed[0].dtype == torch.uint8
    else:
        slots = {B: torch.empty((B,) + img, device=DEV) for B in set(batches)}    # a batch size keeps its address: plans are keyed on it
    losses, paths = [], []
    for step, B in enumerate(batches):
        if u8:
            data = feed[step]
        else:
            data = slots[B]
            data.copy_(torch.rand((B,) + img, generator=gen))
        if loss == "factor":
            Bh = B // 2
            noise = (torch.randn(Bh, D, generator=gen).to(DEV), torch.randn(Bh, D, generator=gen).to(DEV),
                     torch.stack([torch.randperm(Bh, generator=gen) for _ in range(D)]))
        else:
            eps = torch.randn(B, D, generator=gen).to(DEV)
        if poisoned:
            paths = _poison(model, loss_f)
        if loss == "factor":
            l = loss_f.call_optimize(data, model, opt, None, noise=noise)
        else:
            l = loss_f.fused_step(data, model, opt, None, eps=eps)
        losses.append(l.item())
    torch.cuda.synchronize()
    if poisoned:
        _check_walk(paths, model, loss_f, set(batches), loss)
    if replay == "plan":
        assert loss_f._graphs.replays >= (1 if u8 else 2), "the iteration was never replayed (%d)" % loss_f._graphs.replays
    grads = torch.cat([model.arena.view(n, grad=True).reshape(-1) for n in model.arena.shapes])
    return losses, model.arena.flat.clone(), grads.clone()


def _twins(loss, img, D, replay, batches=BATCHES, u8=False):
    if replay == "plan" and not u8:
        # a plan is keyed on the allocation generation, which the first step of every batch size bumps: the five steps record and
        # never replay.  Two more steps (16, 7) replay the plans of steps 4 and 5 -- on buffers poisoned after a batch-size switch
        batches = tuple(batches) + (16, 7)
    clean = _run(loss, img, D, replay, False, batches, u8)
    dirty = _run(loss, img, D, replay, True, batches, u8)
    assert all(l == l for l in clean[0]), clean[0]
    assert clean[0] == dirty[0], "losses differ once the workspace is poisoned: %s vs %s" % (clean[0], dirty[0])
    assert torch.isfinite(dirty[1]).all() and torch.isfinite(dirty[2]).all()
    assert torch.equal(clean[1], dirty[1]), "parameters differ once the workspace is poisoned"
    assert torch.equal(clean[2], dirty[2]), "gradients differ once the workspace is poisoned"


@pytest.mark.parametrize("replay", [None, "plan"], ids=["eager", "plan"])
@pytest.mark.parametrize("img", [(3, 64, 64), (1, 32, 32)], ids=["3x64x64", "1x32x32"])
@pytest.mark.parametrize("loss", ["VAE", "betaH", "betaB", "btcvae", "factor"])
def test_step_on_poisoned_buffers_is_bit_identical(loss, img, replay):
    _twins(loss, img, 10, replay)


@pytest.mark.parametrize("replay", [None, "plan"], ids=["eager", "plan"])
def test_uint8_input_step_on_poisoned_buffers(replay):
    """The DeviceImageLoader path: uint8 batches (16, 16, 7, then the next epoch's 16, 16) consumed by the fused /255 kernels.  Plan
    mode runs into a third epoch: its batches have the addresses AND the allocation generation of the second epoch's, so they
    replay."""
    _twins("btcvae", (3, 64, 64), 10, replay, batches=(16, 16, 7, 16, 16) + ((7, 16, 16) if replay else ()), u8=True)


@pytest.mark.parametrize("loss", ["btcvae", "factor"])
def test_wide_latent_step_on_poisoned_buffers(loss):
    """latent_dim 24: the run-time-D kernels and the wide scal / packed / rowstats layouts."""
    _twins(loss, (3, 64, 64), 24, "plan")
