"""CPU: the launch schedule of VAEEngine.decode_backward / encode_backward -- which launches a backward pass issues, with
which arguments, in which order and on which stream -- for every policy, geometry and both sides of every row threshold
(schedule_trace.AXES), without a GPU and without the library.

test_trace_matches_recorded compares entry by entry with tests/golden/backward_launch_trace.json, recorded once from
commit fe3c759 (the last one before the backward half of engine.py was split into layer descriptions and one function
per policy) and not regenerated since: a launch that moves, changes stream or loses its fork fails here.
test_schedule_invariants states what must hold of ANY schedule, independent of the fixture."""
import itertools
import json
import os

import pytest

import schedule_trace as T

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "backward_launch_trace.json")
GEOMETRIES = list(itertools.product(T.AXES["geometry"], T.AXES["latent_dim"]))
REST = [T.AXES[k] for k in ("rows", "policy", "dtype", "calls")]


def _show(trace):
    return "\n".join("  %2d %s" % (i, e) for i, e in enumerate(trace))


@pytest.mark.parametrize("img,D", GEOMETRIES)
def test_trace_matches_recorded(img, D):
    with open(FIXTURE) as f:
        fx = json.load(f)
    assert fx["axes"] == json.loads(json.dumps(T.AXES)), "the fixture was recorded over other cases"
    n_rest = len(list(itertools.product(*REST)))
    assert len(fx["cases"]) == len(GEOMETRIES) * n_rest
    first = GEOMETRIES.index((img, D)) * n_rest
    tracer = T.Tracer(img, D)
    for i, (B, policy, dtype, calls) in enumerate(itertools.product(*REST)):
        want = [fx["entries"][j] for j in fx["traces"][fx["cases"][first + i]]]
        got = json.loads(json.dumps(tracer.trace(B, policy, dtype, calls)))
        case = "%s D=%d B=%d %s %s %s" % (img, D, B, policy, dtype, calls)
        for k, (g, w) in enumerate(itertools.zip_longest(got, want)):
            assert g == w, "%s: entry %d is\n  %s\nrecorded\n  %s\nthe whole trace:\n%s\nrecorded:\n%s" % (
                case, k, g, w, _show(got), _show(want))


def _operands(e):
    """Tensors a weight-gradient launch reads."""
    if e[0] == T.GROUPED:
        return [t for prob in e[1] for t in prob[:2]]
    return e[1:3] if e[0] == "dvae_conv4s2_wgrad_u8" else [e[1], e[3]]


def _written(e):
    """Gradient tensors a weight-gradient launch writes (its layer's .weight)."""
    if e[0] == T.GROUPED:
        return [prob[2] for prob in e[1]]
    return [e[3] if e[0] == "dvae_conv4s2_wgrad_u8" else e[5]]


@pytest.mark.parametrize("img,D", GEOMETRIES)
def test_schedule_invariants(img, D):
    tracer = T.Tracer(img, D)
    eng = tracer.eng
    dec = ["g:decoder.%s.weight" % n for n in eng.dec_names + ["convT3"]]
    enc = ["g:encoder.%s.weight" % n for n in eng.enc_names]
    dec_fc = ["g:decoder.%s.weight" % n for n in ("lin1", "lin2", "lin3")]
    enc_fc = ["g:encoder.%s.weight" % n for n in ("lin1", "lin2", "mu_logvar_gen")]
    for B, policy, dtype, calls in itertools.product(*REST):
        trace = tracer.trace(B, policy, dtype, calls)
        case = "%s D=%d B=%d %s %s %s:\n%s" % (img, D, B, policy, dtype, calls, _show(trace))
        # what fc_chain_bwd writes: the six FC input gradients and, with the fused 4x4 ends, convT_64's in front and conv_64's behind
        chain = ["gd2", "gd1", "dz", "dml", "gh2", "gh1", "ga_flat"]
        if eng._ends(B):
            chain += ["gd3", "enc_gact[%d]" % (len(eng.enc_names) - 2)]
        single = policy == "single_stream"
        last_write, ws_stream, conv_w, fc_w = {}, {}, [], []
        for i, e in enumerate(trace):
            stream = e[-1]
            if e[0] in T.CONV_WGRADS or e[0] == T.GROUPED:
                (fc_w if e[0] == T.GROUPED else conv_w).extend(_written(e))
                if stream != "main":
                    # a side stream's weight gradient: that stream was ordered behind the main stream AFTER the launch that
                    # produced the last of its operands
                    made = max(last_write.get(t, -1) for t in _operands(e))
                    assert ["dvae_stream_order", "main", stream] in trace[made + 1:i], "entry %d has no fork, %s" % (i, case)
            elif e[0] in T.ROWS_OUT:
                assert stream == "main", "entry %d: an input gradient off the main stream, %s" % (i, case)
                last_write[e[T.ROWS_OUT[e[0]][1] + 1]] = i
            elif e[0] == "fc_chain":
                last_write.update((t, i) for t in chain)
            # one stream per partial-sum workspace
            for ws in ("_ws", "_ws_side", "_ws_wg2"):
                if ws in e[1:]:
                    assert ws_stream.setdefault(ws, stream) == stream, "entry %d: %s on two streams, %s" % (i, ws, case)
        if single:
            assert not any(e[0] == "dvae_stream_order" for e in trace), case
            assert set(ws_stream.values()) <= {"main"}, case
        else:
            assert ws_stream.get("_ws", "main") == "main" and ws_stream.get("_ws_side", "side") == "side" \
                and ws_stream.get("_ws_wg2", "wg2") == "wg2", case
        # every weight gradient of the half / halves that ran, exactly once
        halves = {"decode": (dec, dec_fc), "encode": (enc, enc_fc)}.get(calls, (dec + enc, dec_fc + enc_fc))
        assert sorted(conv_w) == sorted(halves[0]), case
        assert sorted(fc_w) == sorted(halves[1]), case
        # the pass ends with the join of every side stream it used (every call shape here ends on a joining call)
        if not single:
            joins = [["dvae_stream_order", "side", "main"]]
            if any(e[-1] == "wg2" for e in trace):
                joins.append(["dvae_stream_order", "wg2", "main"])
            assert trace[-len(joins):] == joins, case
        # a pending at_next_fork hook fires once, right behind a fork of the side stream
        hooks = [i for i, e in enumerate(trace) if e[0] == "hook"]
        if calls in ("step", "step_nodefer", "autograd_hook") and not single:
            assert len(hooks) == 1 and trace[hooks[0] - 1] == ["dvae_stream_order", "main", "side"], case
        else:
            assert not hooks, case
