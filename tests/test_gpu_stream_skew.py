"""-m gpu: the step does not care which of its streams lags.

tests/test_schedule_hazards.py proves on the CPU that every cross-stream buffer hazard of a step is ordered; this is the same
property on the device.  A missing edge passes every other GPU test because at test sizes the side stream happens to finish
first, so here ONE stream is made to lag on purpose: ``call`` as engine.py, models/losses.py and models/discriminator.py see it
(the three patch points of tests/step_trace.py) enqueues a device-side delay (torch.cuda._sleep: it touches no memory) on the
victim stream in front of every launch that goes to it.  The delay is at least twice the time of a whole unskewed step of that
shape -- measured in the test -- so the victim falls behind everything the other streams have to do.

Per shape: two seeded eager steps (replay off) with every torch.empty buffer NaN-poisoned before each step
(test_gpu_step_poison._poison), once under the single-stream policy (policy_override = every field schedule.build_policy
derives under DVAE_STREAMS=1, single_stream = True among them: all launches serial on one stream, no skew is possible), once
under the default policy without skew (the control: schedule.py promises "the same launches on the same streams, bit-identical
results"), and once per victim stream.  The loss of both steps, the logged scalars, every gradient and the parameters after
Adam must be bit-identical to the single-stream run.

test_dropped_fork_is_noticed is the sensitivity control: with the backward pass's first main -> side fork filtered out of the
wrapped calls and the main stream delayed, the side stream's weight gradient reads what the main stream has not written yet
-- NaN poison -- and the outputs must DIFFER (wrong arithmetic on allocated buffers: every pointer stays valid).
"""
import contextlib
from collections import defaultdict
from unittest import mock

import pytest
import torch

pytestmark = pytest.mark.gpu

from disvae_amd import _lib, engine as E, schedule as SCHED
from disvae_amd.models import discriminator as DISC, losses as L
from test_gpu_step_poison import DEV, _make, _poison

ORDERING = ("dvae_stream_order", "dvae_event_record", "dvae_event_wait")
CASE_BUDGET_MS = 3000.0        # number of delayed launches x delay stays under this
STEPS = 2


def _three_rows(img, D, kind):
    """The smallest row count at which schedule.build_policy turns three_streams on for this loss (None: at no size a step can
    have -- beta-TCVAE's threshold is parked at 1 << 30)."""
    rows = SCHED.THREE_STREAM_MIN_ROWS_FACTOR if kind == _lib.LOSS_FACTOR else SCHED.THREE_STREAM_MIN_ROWS
    if rows > _lib.FC_CHAIN_MAX_ROWS:
        return None
    on = lambda r: SCHED.build_policy(img, D, r, SCHED.switches(), 1, kind).three_streams
    assert on(rows) and not on(rows - 2), rows
    return rows


_BTC3 = _three_rows((3, 64, 64), 10, _lib.LOSS_BTCVAE)
# name -> (loss, geometry, latent_dim, rows, uint8 input, policy fields forced in every run of the case, victim streams)
CASES = {
    "betaH-1x64x64-B16": ("betaH", (1, 64, 64), 10, 16, False, {}, ("side", "main")),
    "btcvae-3x64x64-B16": ("btcvae", (3, 64, 64), 10, 16, False, {}, ("side", "main")),
    # three streams: at the policy's own threshold where a step can reach it, else forced at B = 16 (the same three-queue
    # schedule: schedule_trace's "three_streams" policy)
    "btcvae-3x64x64-three": ("btcvae", (3, 64, 64), 10, _BTC3 or 16, False, {} if _BTC3 else {"three_streams": True},
                             ("side", "wg2", "main")),
    "factor-1x64x64-2x16": ("factor", (1, 64, 64), 10, 32, False, {}, ("side", "main")),
    # the discriminator's second chain on the exchange stream: the only use a single-process FactorVAE step has for it
    "factor-1x64x64-2x16-aux": ("factor", (1, 64, 64), 10, 32, False, {"disc_chain2_aux": True}, ("aux",)),
    "factor-1x64x64-three": ("factor", (1, 64, 64), 10, _three_rows((1, 64, 64), 10, _lib.LOSS_FACTOR), False, {},
                             ("side", "wg2", "main")),
    "btcvae-1x32x32-D17-B16": ("btcvae", (1, 32, 32), 17, 16, False, {}, ("side", "main")),
    "btcvae-3x64x64-B16-uint8": ("btcvae", (3, 64, 64), 10, 16, True, {}, ("side", "main")),
}
SKEWED = [(name, victim) for name, c in CASES.items() for victim in c[6]]


def _raw_streams():
    dev = torch.device(DEV, torch.cuda.current_device())
    side, aux = E.device_streams(dev)
    return {"main": (None, torch._C._cuda_getCurrentRawStream(torch.cuda.current_device())),
            "side": (side, side.cuda_stream), "aux": (aux, aux.cuda_stream),
            "wg2": (E.wg2_stream(dev), E.wg2_stream(dev).cuda_stream)}


@contextlib.contextmanager
def _wrapped_calls(victim=None, cycles=0, drop_first_fork=False, counts=None):
    """_lib.call as seen by engine / losses / discriminator: a delay on `victim` in front of each of its launches; optionally
    the first main -> side dvae_stream_order of every step (the backward pass's first fork in a betaH step) is not issued."""
    streams = _raw_streams()
    handle, raw = streams[victim] if victim else (None, None)
    main_raw, side_raw = streams["main"][1], streams["side"][1]
    state = {"dropped": False}
    real = _lib.call

    def call(name, *args):
        if name == "dvae_stage_weights":          # the head of a step
            state["dropped"] = False
        if name == "dvae_stream_order":
            if drop_first_fork and not state["dropped"] and args == (main_raw, side_raw):
                state["dropped"] = True
                return
        elif name not in ORDERING:
            if counts is not None:
                counts[args[-1]] += 1
            if victim and args[-1] == raw:
                with torch.cuda.stream(handle) if handle is not None else contextlib.nullcontext():
                    torch.cuda._sleep(cycles)
        return real(name, *args)
    with contextlib.ExitStack() as st:
        for mod in (E, L, DISC):
            st.enter_context(mock.patch.object(mod, "call", call))
        yield state


def _single_stream_policy(img, D, B, kind):
    """Every field of the policy schedule.build_policy derives for this step under DVAE_STREAMS=1.  (single_stream alone is
    no consistent policy for the batch-coupled losses: build_policy also turns the late join and the discriminator's side
    streams off with it, and engine.fork_side never runs a deferred epilogue on one stream.)"""
    sw = tuple("1" if name == "DVAE_STREAMS" else v for (name, _), v in zip(SCHED.SWITCHES, SCHED.switches()))
    pol = SCHED.build_policy(tuple(img), D, B, sw, 1, kind, True, None)
    assert pol.single_stream and not pol.late_join and not pol.three_streams
    return pol._asdict()


def _run(case, single=False, **wrap):
    """Two seeded, poisoned eager steps -> (what is compared, milliseconds of each step on the device)."""
    loss, img, D, B, u8, forced, _ = CASES[case]
    model, opt, loss_f = _make(loss, img, D)
    loss_f.replay = None
    loss_f.policy_override = _single_stream_policy(img, D, B, loss_f.KIND) if single else dict(forced)
    gen = torch.Generator().manual_seed(8)
    out, ms = {}, []
    with _wrapped_calls(**wrap):
        for step in range(STEPS):
            if u8:
                data = torch.randint(0, 256, (B,) + img, dtype=torch.uint8, generator=gen).to(DEV)
            else:
                data = torch.rand((B,) + img, generator=gen).to(DEV)
            if loss == "factor":
                Bh = B // 2
                noise = (torch.randn(Bh, D, generator=gen).to(DEV), torch.randn(Bh, D, generator=gen).to(DEV),
                         torch.stack([torch.randperm(Bh, generator=gen) for _ in range(D)]))
            else:
                eps = torch.randn(B, D, generator=gen).to(DEV)
            _poison(model, loss_f)
            storer = defaultdict(list)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            if loss == "factor":
                l = loss_f.call_optimize(data, model, opt, storer, noise=noise)
            else:
                l = loss_f.fused_step(data, model, opt, storer, eps=eps)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
            out["loss %d" % step] = l.detach().clone().reshape(1)
            out["scalars %d" % step] = loss_f._scratch.scal.clone()
            out["logged %d" % step] = torch.tensor([v for k in sorted(storer) for v in storer[k]], dtype=torch.float64)
            out["gradients %d" % step] = torch.cat([model.arena.view(n, grad=True).reshape(-1) for n in model.arena.shapes])
            out["parameters %d" % step] = model.arena.flat.clone()
            if loss == "factor":
                disc = loss_f.discriminator
                out["discriminator gradients %d" % step] = disc.arena.grad.clone()
                out["discriminator parameters %d" % step] = disc.arena.flat.clone()
    return out, ms


def _differences(a, b):
    """Names of the compared tensors that are not bit-identical (NaN equals NaN: the bits are what counts)."""
    assert a.keys() == b.keys()
    return [k for k in a if not torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k],
                                            b[k].view(torch.int32) if b[k].dtype == torch.float32 else b[k])]


_REF, _CYCLES_PER_MS = {}, []


def _reference(case):
    """(the single-stream run, the unskewed default run, its step times, launches per raw stream of its steps): once per case."""
    if case not in _REF:
        single, _ = _run(case, single=True)
        counts = defaultdict(int)
        plain, ms = _run(case, counts=counts)
        assert all(torch.isfinite(v).all() for v in single.values()), case
        assert len(single["logged 0"]) >= 3, "the first step logged nothing"
        _REF[case] = (single, plain, ms, counts)
    return _REF[case]


def _cycles_per_ms():
    """What torch.cuda._sleep counts, measured: cycles per millisecond of delay."""
    if not _CYCLES_PER_MS:
        best = 0.0
        for n in (1 << 20, 1 << 24):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            torch.cuda._sleep(n)
            e1.record()
            torch.cuda.synchronize()
            best = n / max(e0.elapsed_time(e1), 1e-3)
        _CYCLES_PER_MS.append(best)
    return _CYCLES_PER_MS[0]


def _delay(case, victim):
    """(cycles, milliseconds) of one delay: twice the unskewed step, capped so that the whole case stays under CASE_BUDGET_MS."""
    _, _, ms, counts = _reference(case)
    step_ms = ms[-1]                                   # the second step: buffers allocated, kernels loaded
    n = max(counts[_raw_streams()[victim][1]], 1)      # launches on the victim over both steps
    assert counts[_raw_streams()[victim][1]] > 0, "%s: no launch goes to %s" % (case, victim)
    want = 2.0 * step_ms
    delay_ms = min(want, CASE_BUDGET_MS / n)
    return int(delay_ms * _cycles_per_ms()) + 1, delay_ms, step_ms, n


@pytest.mark.parametrize("case", list(CASES))
def test_default_policy_equals_single_stream(case):
    """The unskewed control: a difference here is the policy's, not the skew's."""
    single, plain, ms, counts = _reference(case)
    assert _differences(single, plain) == [], "%s: default policy vs single stream" % case
    if "three" in case:
        assert counts[_raw_streams()["wg2"][1]] > 0, "the case does not reach the three-stream schedule"


@pytest.mark.parametrize("case,victim", SKEWED, ids=["%s-%s" % cv for cv in SKEWED])
def test_step_does_not_care_which_stream_lags(case, victim):
    assert hasattr(torch.cuda, "_sleep")
    single, _, ms, _ = _reference(case)
    cycles, delay_ms, step_ms, n = _delay(case, victim)
    skewed, skewed_ms = _run(case, victim=victim, cycles=cycles)
    print("%s victim %s: unskewed steps %s ms, %d delayed launches x %.3f ms (%d cycles, wanted %.3f ms), skewed steps %s ms"
          % (case, victim, ["%.3f" % v for v in ms], n, delay_ms, cycles, 2.0 * step_ms, ["%.3f" % v for v in skewed_ms]))
    assert skewed_ms[-1] > ms[-1] + delay_ms, "the delay did nothing: %.3f ms against %.3f ms unskewed" % (skewed_ms[-1], ms[-1])
    assert _differences(single, skewed) == [], "%s with %s lagging %.3f ms per launch" % (case, victim, delay_ms)


def test_dropped_fork_is_noticed():
    """Sensitivity: without the backward pass's first main -> side fork (tests/test_schedule_hazards.py: not redundant) and with
    the main stream lagging, convT3's weight gradient on the side stream reads g_logit before the forward pass has written it."""
    case = "betaH-1x64x64-B16"
    single, _, ms, _ = _reference(case)
    cycles, delay_ms, _, _ = _delay(case, "main")
    with_fork, _ = _run(case, victim="main", cycles=cycles)
    assert _differences(single, with_fork) == []
    broken, _ = _run(case, victim="main", cycles=cycles, drop_first_fork=True)
    diff = _differences(single, broken)
    print("without the first fork, main lagging %.3f ms per launch: %s differ" % (delay_ms, diff))
    assert any(k.startswith("gradients") for k in diff), "the skew does not expose a missing fork: nothing differs"
