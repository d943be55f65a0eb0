"""CPU: the launch sequence of one whole native step -- loss_f.fused_step / FactorKLoss.call_optimize, from engine.stage to the
final join or all-reduce: every launch, collective and ordering edge, its arguments and its stream -- for every loss, training
and evaluation, single process and both ranks of two, both estimator scopes and every debug switch (step_trace.AXES, minus
step_trace.dropped), without a GPU and without the library.

test_step_trace_matches_recorded compares entry by entry with tests/golden/step_launch_trace.json, recorded once from
commit 6d5b14e (the last one before models/losses.py was reorganised into one step skeleton) and not regenerated since.
test_step_invariants states what must hold of ANY step, independent of the fixture.  Its invariant 1 (a launch off the main
stream is ordered behind the main-stream launch that wrote its newest operand) is one direction of one kind of hazard; the
general form -- every cross-stream read-after-write, write-after-read and write-after-write, from any stream, workspaces
included -- is tests/test_schedule_hazards.py."""
import itertools
import json
import os

import pytest

import step_trace as S

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_launch_trace.json")
MODELS = S.AXES["model"]


def _show(trace):
    return "\n".join("  %2d %s" % (i, e) for i, e in enumerate(trace))


def _label(case):
    loss, mode, (img, D), rows, dtype, world, estimator, noise, switch = case
    return "%s %s %s D=%d B=%d %s world=%d rank=%d %s %s %s" % ((loss, mode, img, D, rows, dtype) + tuple(world)
                                                                  + (estimator, noise, switch))


def _cases_of(model):
    """(number in the fixture, case) of every case of one model."""
    return [(i, c) for i, c in enumerate(S.cases()) if c[2] == model]


@pytest.mark.parametrize("model", MODELS)
def test_step_trace_matches_recorded(model):
    with open(FIXTURE) as f:
        fx = json.load(f)
    assert fx["axes"] == json.loads(json.dumps(S.AXES)), "the fixture was recorded over other cases"
    assert len(fx["cases"]) == len(list(S.cases()))
    tracer = S.StepTracer(*model)
    for i, case in _cases_of(model):
        want = S.unpack(fx, i)
        got = json.loads(json.dumps(tracer.trace(*(case[:2] + case[3:]))))
        for k, (g, w) in enumerate(itertools.zip_longest(got, want)):
            assert g == w, "%s: entry %d is\n  %s\nrecorded\n  %s\nthe whole trace:\n%s\nrecorded:\n%s" % (
                _label(case), k, g, w, _show(got), _show(want))


# ---- what a launch touches ------------------------------------------------------------------------------------------------
# entry -> positions (among its arguments) of the buffers it writes
WRITES = {
    "dvae_stage_weights": (3,), "dvae_conv32_down": (4,), "dvae_conv32_up": (5,), "dvae_conv32_up_bits": (4, 5),
    "dvae_conv1_fwd_bits": (4, 5), "dvae_conv4s2_fwd_u8": (3,), "dvae_conv4s2_fwd": (4,), "dvae_linear_fwd": (3,),
    "dvae_reparam_kl_fwd": (2, 3, 4, 5), "dvae_reparam_kl_bwd": (10,), "dvae_convT3_fwd_staged": (5, 6, 9),
    "dvae_convT4s2_sigmoid_recon_fwd_u8": (4, 5, 8), "dvae_convT4s2_sigmoid_recon_fwd": (5, 6, 9), "dvae_u8_to_f32": (1,),
    "dvae_loss_epilogue": (2, 10, 11), "dvae_loss_finalize": (5,), "dvae_loss_pack": (6,), "dvae_kl_finish": (0,),
    "dvae_btcvae_fwd": (9, 10), "dvae_btcvae_bwd": (11, 12, 13, 14), "dvae_permute_dims": (2,), "dvae_disc_losses": (3, 4, 5),
    "dvae_linear_dgrad": (4,), "dvae_linear_wgrad": (2, 3), "dvae_convT4s2_wgrad": (4, 5), "dvae_conv4s2_wgrad": (4, 5),
    "dvae_conv4s2_wgrad_u8": (2, 3), "dvae_convT3_dgrad_bits": (3,), "dvae_convT4s2_dgrad": (4,), "scale_": (0,),
    "copy_flat_": (0,), "py": (1,), "all_gather_latents": (3,), "all_gather_rows": (1,),
}
FC_FWD = ["h1", "h2", "ml", "mu", "logvar", "z", "kl_dim", "d1", "d2", "d3"]        # + convT_out
FC_BWD = ["gd2", "gd1", "dz", "dml", "gh2", "gh1", "ga_flat"]                       # + gd3 and conv_gin with the fused 4x4 ends
ORDERING = ("dvae_stream_order", "dvae_event_record", "dvae_event_wait", "wait")
COLLECTIVES = ("all_reduce", "all_reduce_async", "all_reduce_cols_sums")
NOT_BUFFERS = {"B", "WB", "Bh", "2Bh", "WBh", "slot", "all", "numel(x)", "main", "side", "aux", "wg2", "normal_", "copy_",
               "_ws", "_ws_side", "_ws_wg2", "disc._wsbuf", "disc._wsbuf_side", "disc._wsbuf_aux"}


def _base(s):
    return s.split("+")[0]


def _strings(v):
    if isinstance(v, list):
        for u in v:
            yield from _strings(u)
    elif isinstance(v, str):
        yield v


def _touched(e):
    """Every buffer an entry names (launches off the main stream: none of them takes an argument struct)."""
    return {_base(s) for s in _strings(e[1:]) if s not in NOT_BUFFERS and not s.startswith(("klb(", "1/("))}


def _written(e):
    name = e[0]
    if name == "dvae_fc_chain_fwd":
        return FC_FWD + [_base(v) for k, v in e[1][1:] if k == "convT_out"]
    if name == "dvae_fc_chain_bwd":
        f = dict(e[1][1:])
        return FC_BWD + (["gd3", _base(f["conv_gin"])] if "convT_gout" in f else [])
    if name == S.T.GROUPED:
        return [t for prob in e[1] for t in prob[2:4]]
    if name in COLLECTIVES:
        return [_base(e[1][0])]
    return [_base(e[i + 1]) for i in WRITES.get(name, ()) if isinstance(e[i + 1], str)]


def _reach(trace, lo, hi, start):
    """Streams ordered behind everything stream `start` holds at position lo, by the ordering entries of trace[lo:hi]: a
    dvae_stream_order, an event slot recorded and waited for, or an asynchronous collective started and waited for."""
    reach, marks = {start}, set()
    for e in trace[lo:hi]:
        if e[0] == "dvae_stream_order" and e[1] in reach:
            reach.add(e[2])
        elif e[0] in ("dvae_event_record", "all_reduce_async") and e[-1] in reach:
            marks.add(json.dumps(e[1]))
        elif e[0] in ("dvae_event_wait", "wait") and json.dumps(e[1]) in marks:
            reach.add(e[-1])
    return reach


def _check(tracer, case, trace):
    loss, mode, _, rows, dtype, (world, rank), estimator, noise, switch = case
    where = "%s:\n%s" % (_label(case), _show(trace))
    train = mode == "train"
    names = [e[0] for e in trace]
    index = lambda pred: [i for i, e in enumerate(trace) if pred(e)]

    # 1. a launch or collective off the main stream: since the main-stream launch that produced its newest operand, that
    #    stream was ordered behind the main stream (directly, or main -> side -> aux)
    main_write = {}
    for i, e in enumerate(trace):
        stream = e[-1]
        if e[0] in ORDERING:
            continue
        if stream != "main":
            made = max([main_write.get(b, -1) for b in _touched(e)] + [-1])
            if made >= 0:
                assert stream in _reach(trace, made + 1, i, "main"), "entry %d is not ordered behind entry %d, %s" % (i, made, where)
        for b in _written(e):
            if stream == "main":
                main_write[b] = i

    # 2. every wait for the event slot follows exactly one record of it
    for i in index(lambda e: e[0] == "dvae_event_wait"):
        assert names[:i].count("dvae_event_record") == 1, "entry %d, %s" % (i, where)

    # 4. the scalar losses are finalised exactly once
    final = index(lambda e: (e[0] == "dvae_loss_epilogue" and e[12] is not None) or e[0] == "dvae_loss_finalize")
    assert len(final) == 1, where

    # 3. the FC chain's input gradients come behind the scalar loss and (beta-TCVAE) the estimator's backward
    if train:
        chain = index(lambda e: e[0] in ("dvae_fc_chain_bwd", "dvae_reparam_kl_bwd"))
        assert len(chain) == 1 and trace[chain[0]][-1] == "main", where
        first = final + (index(lambda e: e[0] == "dvae_btcvae_bwd") if loss == "btcvae" else [])
        assert len(first) == (2 if loss == "btcvae" else 1), where
        for p in first:
            assert p < chain[0] and "main" in _reach(trace, p + 1, chain[0], trace[p][-1]), \
                "the FC chain (entry %d) is not ordered behind entry %d, %s" % (chain[0], p, where)

    # 6. sharded: the packed loss sums are all-reduced exactly once, between pack and finalize
    if world > 1:
        fin = trace[final[0]]
        assert fin[0] == "dvae_loss_finalize", where
        pk = _base(fin[2])
        packs = index(lambda e: (e[0] == "dvae_loss_epilogue" and e[12] is None and _base(e[11]) == pk)
                      or (e[0] == "dvae_loss_pack" and _base(e[7]) == pk))
        sums = index(lambda e: e[0] in COLLECTIVES and _base(e[1][0]) == pk)
        assert len(packs) == 1 and len(sums) == 1 and packs[0] < sums[0] < final[0], where
        assert trace[packs[0]][-1] == trace[sums[0]][-1] == fin[-1], where

    # 5. sharded training: every gradient is summed over the ranks by exactly one all-reduce, issued behind its last writer
    if world > 1 and train:
        arenas = [("g:", tracer.eng.arena)] + ([("dg:", tracer.disc_arena)] if loss == "factor" else [])
        for prefix, arena in arenas:
            reduces = [(i, arena.offsets[e[1][0][len(prefix):]][0], e[1][1]) for i, e in enumerate(trace)
                       if e[0] in ("all_reduce", "all_reduce_async") and e[1][0].startswith(prefix)]
            for k, (off, n) in arena.offsets.items():
                cover = [i for i, lo, length in reduces if lo <= off and off + n <= lo + length]
                assert len(cover) == 1, "%s%s is covered by %d all-reduces, %s" % (prefix, k, len(cover), where)
                writers = [(j, e[-1]) for j, e in enumerate(trace) if e[0] not in COLLECTIVES and prefix + k in _written(e)]
                assert writers, "%s%s is never written, %s" % (prefix, k, where)
                for j, stream in writers:
                    assert j < cover[0] and trace[cover[0]][-1] in _reach(trace, j + 1, cover[0], stream), \
                        "all-reduce %d is not ordered behind the gradient of entry %d, %s" % (cover[0], j, where)

    # 7. the step ends with every stream it used ordered into the main stream
    for stream in {e[-1] for e in trace if e[0] not in ORDERING} - {"main"}:
        last = max(i for i, e in enumerate(trace) if e[-1] == stream and e[0] not in ORDERING)
        assert "main" in _reach(trace, last + 1, len(trace), stream), "stream %s is not joined, %s" % (stream, where)

    # 8. DVAE_STREAMS=1 (single process: sharded steps keep their streams): no ordering edge, no event slot
    if switch == "DVAE_STREAMS=1" and world == 1:
        assert not any(n in ORDERING for n in names), where
        assert {e[-1] for e in trace} == {"main"}, where


@pytest.mark.parametrize("model", MODELS)
def test_step_invariants(model):
    tracer = S.StepTracer(*model)
    for _, case in _cases_of(model):
        trace = json.loads(json.dumps(tracer.trace(*(case[:2] + case[3:]))))
        _check(tracer, case, trace)
