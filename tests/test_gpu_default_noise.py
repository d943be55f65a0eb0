"""-m gpu: the training step that draws its own noise, eager and replayed, against the step fed with the same draws.

Every other parity test injects the noise (fused_step(..., eps=...), call_optimize(..., noise=...)); Trainer and bench.py never
do.  The self-drawing step runs code of its own: the recorded eps.normal_ into a scratch buffer, FactorVAE's two half draws
and its discarded full-batch draw (quirk Q4, training.py), the ring of pinned permutation buffers with its events, and on
replay the re-issued draws between the recorded launches (plan) or torch's graph-safe Philox offsets (hipGraph).

The injected step is pinned to the fp64 oracle and the golden vectors (tests/test_gpu_step.py), so every case here is two twins
built from the same seed:

  I  injected, eager (replay = None): fed what tests/default_noise.predraw drew with plain torch.randn / torch.randperm from
     seeded generators in the reference's order (that order is pinned on the CPU by tests/test_default_noise_host.py);
  D  default: both generators re-seeded, then Trainer._train_iteration_async(data, storer) with nothing injected.

Same kernels on the same numbers: everything compared is BIT-IDENTICAL -- no tolerance anywhere in this file.  Compared, in this
order (the first two make a failure readable): the noise buffer the engine used in the last step of each batch size against
the pre-drawn noise; both generator states after twin D against the states after the pre-draw; then the per-step losses, the
parameters and Adam's second moments (FactorVAE: of the discriminator too).
"""
import logging
from collections import defaultdict, namedtuple

import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import DEV
from default_noise import predraw, seed as seed_generators, rng_states
from test_gpu_step import _native, HP
from test_gpu_stream_skew import _cycles_per_ms
from disvae_amd.models.vae import init_specific_model
from disvae_amd.models.losses import get_loss_f, FactorKLoss
from disvae_amd.training import Trainer

LOSSES = ["VAE", "betaH", "betaB", "btcvae", "factor"]
IMG = (1, 64, 64)
N_DATA, LR = 737280, 5e-4
MODEL_SEED, DATA_SEED, DEV_SEED, CPU_SEED = 33, 8, 1234, 4321

Twin = namedtuple("Twin", "losses state loss_f ptrs")


def _model(D):
    """Seeded native model in train mode (initialisation consumes the CPU generator: always before predraw / re-seeding)."""
    torch.manual_seed(MODEL_SEED)
    model = init_specific_model("Burgess", IMG, D)
    return model.to(DEV).train()


def _build(loss, D, save_dir):
    if D == 10:
        model, opt, loss_f = _native(loss, IMG, MODEL_SEED, N_DATA, LR)
    else:
        model = _model(D)
        opt = torch.optim.Adam(model.parameters(), lr=LR)
        loss_f = get_loss_f(loss, n_data=N_DATA, device=torch.device(DEV), **dict(HP, latent_dim=D))
    # both twins go through Trainer's constructor: the same optimizer configuration on both sides
    tr = Trainer(model, opt, loss_f, device=torch.device(DEV), logger=logging.getLogger("noise"), save_dir=str(save_dir),
                 is_progress_bar=False)
    return model, opt, loss_f, tr


def _batches(sizes, on_device=False):
    gen = torch.Generator().manual_seed(DATA_SEED)            # test data: a private generator, never the global ones
    out = [torch.rand((B,) + IMG, generator=gen) for B in sizes]
    return [x.to(DEV) for x in out] if on_device else out


def _second_moments(opt):
    return torch.cat([opt.state[p]["exp_avg_sq"].reshape(-1) for g in opt.param_groups for p in g["params"]])


def _state(model, opt, loss_f):
    out = {"parameters": model.arena.flat.clone(), "exp_avg_sq": _second_moments(opt), "n_train_steps": loss_f.n_train_steps}
    if isinstance(loss_f, FactorKLoss):
        out["discriminator parameters"] = loss_f.discriminator.arena.flat.clone()
        out["discriminator exp_avg_sq"] = _second_moments(loss_f.optimizer_d)
    return out


def _run(loss, built, batches, noise=None, mode=None, feed="static", hold=0, storer=True, before_step=None):
    """One twin (`built`: what _build returned -- building seeds the generators, so it happens before the pre-draw) over
    `batches`: I when `noise` is given (eager, fed with it), else D (replay = `mode`, draws for itself; the caller seeds).
    feed "static": each batch is copied into ONE device tensor per batch size (plans and graphs are keyed on its address);
    "fresh": a new device tensor per step, the first `hold` kept alive and then released together."""
    injected = noise is not None
    model, opt, loss_f, tr = built
    loss_f.replay = None if injected else mode
    losses, ptrs, held, static = [], [], [], {}
    data = None
    for i, x in enumerate(batches):
        if before_step is not None:
            before_step(i)
        if feed == "static":
            if x.shape[0] not in static:
                static[x.shape[0]] = torch.empty(x.shape, device=DEV)
            data = static[x.shape[0]]
            data.copy_(x, non_blocking=True)
        else:
            data = x.to(DEV)
            if i < hold:
                held.append(data)
            else:
                del held[:]
        ptrs.append(data.data_ptr())
        st = defaultdict(list) if storer else None
        if not injected:
            l = tr._train_iteration_async(data, st)
        elif loss == "factor":
            n = noise[i]
            l = loss_f.call_optimize(data, model, opt, st, noise=(n["eps1"], n["eps2"], n["perms"]))
        else:
            l = loss_f.fused_step(data, model, opt, st, eps=noise[i]["eps"])
        losses.append(l.clone())                  # sc.scal is reused by the next step: cloned on the device, no host sync
    torch.cuda.synchronize()
    return Twin(torch.stack(losses), _state(model, opt, loss_f), loss_f, ptrs)


def _used_noise(loss_f, loss, B, D):
    """The noise buffer the engine's self-drawing step of batch size B wrote (never allocated here)."""
    sc = loss_f._scratch
    key = ("eps12", 2 * (B // 2), D) if loss == "factor" else ("eps", B, D)
    assert key in sc.lat, "the step never drew into %r: %s" % (key, sorted(sc.lat))
    got = loss_f.scratch(sc.device).for_latent_dim(D).latent(*key)
    assert got is sc.lat[key]
    return got


def _fed_noise(loss, n):
    return torch.cat([n["eps1"], n["eps2"]]) if loss == "factor" else n["eps"]


def _assert_twins(loss, D, sizes, noise, states, I, Dd, what):
    for B in sorted(set(sizes)):
        last = max(i for i, b in enumerate(sizes) if b == B)
        assert torch.equal(_used_noise(Dd.loss_f, loss, B, D), _fed_noise(loss, noise[last])), \
            "%s: the noise the engine used in step %d (batch %d) is not the pre-drawn one" % (what, last, B)
    dev_state, cpu_state = rng_states(DEV)
    assert torch.equal(dev_state, states[0]), "%s: device generator consumed differently than the reference's draws" % what
    assert torch.equal(cpu_state, states[1]), "%s: CPU generator consumed differently than the reference's draws" % what
    assert torch.equal(I.losses, Dd.losses), "%s: losses %s vs %s" % (what, I.losses.tolist(), Dd.losses.tolist())
    assert I.state.keys() == Dd.state.keys()
    for k, v in I.state.items():
        same = torch.equal(v, Dd.state[k]) if torch.is_tensor(v) else v == Dd.state[k]
        assert same, "%s: %s differ" % (what, k)
    assert torch.isfinite(I.losses).all()


def _twins(loss, D, sizes, mode, tmp_path, what, batches=None, **kw):
    """Order: both models built (their initialisation seeds and consumes the CPU generator), pre-draw (seeds), twin I, re-seed,
    twin D, compare.  -> (I, D, noise)"""
    batches = _batches(sizes) if batches is None else batches
    built_i, built_d = _build(loss, D, tmp_path / "I"), _build(loss, D, tmp_path / "D")
    noise, dev_state, cpu_state = predraw(loss, sizes, D, DEV_SEED, CPU_SEED, DEV)
    kw_i = dict(kw, before_step=None)
    I = _run(loss, built_i, batches, noise=noise, **kw_i)
    seed_generators(DEV_SEED, CPU_SEED, DEV)
    Dd = _run(loss, built_d, batches, mode=mode, **kw)
    _assert_twins(loss, D, sizes, noise, (dev_state, cpu_state), I, Dd, what)
    return I, Dd, noise


# ---- a. every loss, eager and both replay modes ------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [None, "plan", "graph"], ids=["eager", "plan", "graph"])
@pytest.mark.parametrize("loss", LOSSES)
def test_every_loss_every_mode(loss, mode, tmp_path):
    """8 steps, a fresh batch copied into one static device tensor each step.  FactorVAE at B = 17: half batch 8, one row
    dropped, the discarded Q4 draw has 17 rows.  (hipGraph: 9 steps -- the first step allocates the engine's buffers, which
    changes the graph's key, then StepGraphs.WARMUP = 2 eager steps and the capture: the fifth counted replay is step 9.)"""
    B = 17 if loss == "factor" else 16
    steps = 9 if mode == "graph" else 8
    _, Dd, _ = _twins(loss, 10, [B] * steps, mode, tmp_path, "%s %s" % (loss, mode))
    if mode:
        assert Dd.loss_f._graphs.replays >= 5, "the iteration was not replayed: %d" % Dd.loss_f._graphs.replays


# ---- b. batches as the Trainer really gets them -------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", ["btcvae", "factor"])
def test_fresh_batch_tensors_and_recurring_addresses(loss, tmp_path):
    """A new device tensor per step under the shipped default ("auto": a plan at this size).  The first five batches stay alive
    (five plans recorded, one per address), then they are released together: the allocator hands their addresses out again, so
    later steps replay OLDER plans under a recurring pointer."""
    B = 17 if loss == "factor" else 16
    _, Dd, _ = _twins(loss, 10, [B] * 10, "auto", tmp_path, "%s fresh tensors" % loss, feed="fresh", hold=5)
    assert len(set(Dd.ptrs[:5])) == 5
    assert len(set(Dd.ptrs)) < len(Dd.ptrs), "no batch address recurred: %s" % [hex(p) for p in Dd.ptrs]
    assert Dd.loss_f._graphs.replays >= 1, "no plan was replayed under a recurring batch pointer"


# ---- c. the short last batch --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", ["btcvae", "factor"])
def test_short_last_batch(loss, tmp_path):
    """No drop_last in the reference's loaders: 16, 16, 16, 7, 16, 16, 7.  FactorVAE at 7: half batch 3, Q4 draw of 7 rows."""
    sizes = [16, 16, 16, 7, 16, 16, 7]
    _, Dd, _ = _twins(loss, 10, sizes, "auto", tmp_path, "%s short last batch" % loss)
    a, b = (_used_noise(Dd.loss_f, loss, B, 10) for B in (16, 7))
    assert a.data_ptr() != b.data_ptr() and a.shape[0] != b.shape[0], "the two batch sizes share a noise buffer"


# ---- d. the host runs ahead of the permutation ring ---------------------------------------------------------------------------
WARM = 2


@pytest.mark.parametrize("mode", [None, "plan"], ids=["eager", "plan"])
def test_host_runs_ahead_of_the_permutation_ring(mode, tmp_path):
    """12 steps (three times FactorKLoss._PERM_RING) issued with no host synchronisation in between (storer = None, losses kept
    as cloned device scalars, batches resident on the device) behind ONE device-side delay of ~50 ms, so the host is steps ahead
    of the GPU when the ring wraps: a slot overwritten before its host-to-device copy ran would hand a later step's
    permutations to an earlier one.  Twin I gets the same permutation sets as ordinary tensors.

    The delay starts the 12 steps; WARM = 2 ordinary steps (compared like the rest) come before it, because the very first step
    synchronises the host on its own (Adam's launch table reads the step counts back, scratch and pinned buffers are allocated):
    behind the delay it would wait the delay out and the host would never get ahead."""
    n = WARM + 3 * FactorKLoss._PERM_RING
    assert n == WARM + 12
    batches = _batches([16] * n, on_device=True)
    cycles = int(50.0 * _cycles_per_ms())
    torch.cuda.synchronize()
    seen = {}

    def before_step(i):
        if i == WARM:
            torch.cuda._sleep(cycles)                # one call, bounded: a delay, not a fault
            seen["after"] = torch.cuda.Event()
            seen["after"].record()
        elif i == WARM + FactorKLoss._PERM_RING:
            # a full turn of the ring has been issued since the delay began
            seen["ahead"] = not seen["after"].query()
    _twins("factor", 10, [16] * n, mode, tmp_path, "factor ring %s" % mode, batches=batches, storer=False,
           before_step=before_step)
    assert seen["ahead"], "the host never ran ahead of the GPU: the ring was not under test"


# ---- e. wide latent -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [None, "plan"], ids=["eager", "plan"])
def test_wide_latent(mode, tmp_path):
    """D = 20: the run-time-D path hands eps to per-layer launches, not to the fused chain."""
    _twins("btcvae", 20, [16] * 4, mode, tmp_path, "btcvae D=20 %s" % mode)


# ---- f. evaluation draws nothing ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", LOSSES)
def test_evaluation_draws_nothing(loss, tmp_path):
    """One step in eval mode (the call Evaluator.compute_losses makes) leaves both generators where they were, and the
    training step after it is twin I's first step as if the evaluation had not happened."""
    B, D = (17 if loss == "factor" else 16), 10
    (x,) = _batches([B])
    built_i = _build(loss, D, tmp_path / "I")
    model, opt, loss_f, tr = _build(loss, D, tmp_path / "D")
    noise, dev_state, cpu_state = predraw(loss, [B], D, DEV_SEED, CPU_SEED, DEV)
    I = _run(loss, built_i, [x], noise=noise)

    seed_generators(DEV_SEED, CPU_SEED, DEV)
    before = rng_states(DEV)
    data = x.to(DEV)
    model.eval()
    storer = defaultdict(list)
    if loss == "factor":
        loss_f.call_optimize(data, model, None, storer)
    else:
        loss_f.fused_step(data, model, None, storer)
    torch.cuda.synchronize()
    after = rng_states(DEV)
    assert torch.equal(before[0], after[0]), "evaluation consumed the device generator"
    assert torch.equal(before[1], after[1]), "evaluation consumed the CPU generator"
    assert "loss" in storer and loss_f.n_train_steps == 0
    model.train()
    l = tr._train_iteration_async(data, defaultdict(list)).clone()
    torch.cuda.synchronize()
    Dd = Twin(l.reshape(1), _state(model, opt, loss_f), loss_f, [data.data_ptr()])
    _assert_twins(loss, D, [B], noise, (dev_state, cpu_state), I, Dd, "%s after an evaluation" % loss)


# ---- g. the autograd-compatible call surface ----------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [10, 20])
def test_model_call_takes_the_same_single_draw(D):
    """recon, dist, z = model(data) in train mode: one [B, D] draw from the device generator (vae.py:67)."""
    B = 16
    model = _model(D)
    data = _batches([B])[0].to(DEV)
    noise, dev_state, cpu_state = predraw("VAE", [B], D, DEV_SEED, CPU_SEED, DEV)
    with torch.no_grad():
        want = model(data, eps=noise[0]["eps"])[2].clone()
        seed_generators(DEV_SEED, CPU_SEED, DEV)
        recon, (mu, logvar), got = model(data)
    states = rng_states(DEV)
    assert torch.equal(states[0], dev_state) and torch.equal(states[1], cpu_state)
    assert torch.equal(got, want)
    assert not torch.equal(got, mu), "z is the mean: nothing was drawn"
