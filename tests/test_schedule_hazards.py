"""CPU: every cross-stream buffer hazard of a step is ordered -- the general form of the ordering invariants that
test_step_schedule.py and test_backward_schedule.py state for a few named consumers.

For every case of step_trace.cases() and of schedule_trace.AXES, the trace and the trace twice back to back (two steps, with
what the host does in between: the logging read of the scalars, the optimizers, the next batch) go through
hazard_util.check: two entries on different streams that touch the same buffer, one of them writing, must be ordered by
program order and the trace's ordering entries -- read-after-write, write-after-read and write-after-write alike, whichever
stream the earlier one is on, workspaces included.  The rule and how to read a failure: DESIGN.md, "Streams and the late join".

The checker itself is tested on synthetic traces (each kind of missing edge is reported as what it is, the restored trace
passes) and on real traces with one ordering entry filtered out."""
import itertools
import json

import pytest

import hazard_util as H
import schedule_trace as T
import step_trace as S
import test_step_schedule as TS

MODELS = S.AXES["model"]
GEOMETRIES = list(itertools.product(T.AXES["geometry"], T.AXES["latent_dim"]))
REST = [T.AXES[k] for k in ("rows", "policy", "dtype", "calls")]

# Pairs that are safe for a reason a trace cannot express: (earlier entry name, later entry name, base buffer) -> one sentence with
# the file and line that make it true.  At most MAX_EXEMPT rows, none on a workspace or a gradient arena; every row must be hit.
# (None is needed: the extents hazard_util derives -- arena offsets, rows x width, collective spans -- separate every pair of
# launches that share a buffer without sharing data.)
EXEMPT = {}
MAX_EXEMPT = 8


def _hazards(trace, ctx, hit=None):
    out = []
    for h in H.check(trace, ctx):
        key = (trace[h.i][0], trace[h.j][0], h.buf)
        if key in EXEMPT:
            if hit is not None:
                hit.add(key)
        else:
            out.append(h)
    return out


# ---- the two harnesses -------------------------------------------------------------------------------------------------------
def _step_ctx(tracer, case):
    loss, mode, (img, D), rows, dtype, (world, rank), estimator, noise, switch = case
    arenas = {"g:": tracer.eng.arena, "p:": tracer.eng.arena, "dg:": tracer.disc_arena, "dp:": tracer.disc_arena}
    return H.Context(arenas, {"B": rows, "Bh": rows // 2, "D": D, "W": world})


def _step_traces(tracer, case):
    """(label, trace) of one case: the step, and two steps back to back."""
    loss, mode = case[:2]
    one = json.loads(json.dumps(tracer.trace(*(case[:2] + case[3:]))))
    yield TS._label(case), one
    yield TS._label(case) + ", two steps", one + H.between_steps(one, mode == "train", loss == "factor") + one


def _sched_ctx(tracer, B):
    """The context of one backward pass; what the "fc_chain" marker stands for (engine.fc_chain_bwd over B rows)."""
    eng = tracer.eng
    reads = ["d2", "d1", "h2", "h1", "a_flat", "mu", "logvar"]
    writes = ["gd2", "gd1", "dz", "dml", "gh2", "gh1", "ga_flat"]
    if eng._ends(B):      # the fused 4x4 ends: convT_64's input gradient in front of the chain, conv_64's behind it
        k = len(eng.enc_names) - 2
        reads += ["dec_gact[0]", "d3", "enc_act[%d]" % k]
        writes += ["gd3", "enc_gact[%d]" % k]
    else:
        reads.append("gd3")
    return H.Context({"g:": eng.arena, "p:": eng.arena}, {"B": B, "D": tracer.D}, (reads, writes))


def _sched_traces(tracer, rest):
    B, policy, dtype, calls = rest
    label = "%s D=%d B=%d %s %s %s" % ((tracer.img, tracer.D) + tuple(rest))
    one = json.loads(json.dumps(tracer.trace(B, policy, dtype, calls)))
    yield label, one
    yield label + ", two passes", one + one


@pytest.mark.parametrize("model", MODELS)
def test_step_hazards_are_ordered(model):
    tracer = S.StepTracer(*model)
    n = 0
    for _, case in TS._cases_of(model):
        ctx = _step_ctx(tracer, case)
        for label, trace in _step_traces(tracer, case):
            found = _hazards(trace, ctx)
            assert not found, H.describe(label, trace, found)
            n += 1
    assert n == 2 * len(TS._cases_of(model)) > 0


@pytest.mark.parametrize("img,D", GEOMETRIES)
def test_backward_hazards_are_ordered(img, D):
    tracer = T.Tracer(img, D)
    for rest in itertools.product(*REST):
        traces = list(_sched_traces(tracer, rest))      # (the context reads the policy the trace ran under)
        ctx = _sched_ctx(tracer, rest[0])
        for label, trace in traces:
            found = _hazards(trace, ctx)
            assert not found, H.describe(label, trace, found)


# ---- the access table ----------------------------------------------------------------------------------------------------------
def _all_entries():
    """Every distinct entry of every traced case of both harnesses, with a context that resolves its names."""
    seen = set()
    tracers = {}
    for case in S.cases():
        tr = tracers.get(case[2]) or tracers.setdefault(case[2], S.StepTracer(*case[2]))
        ctx = _step_ctx(tr, case)
        for e in json.loads(json.dumps(tr.trace(*(case[:2] + case[3:])))):
            k = (json.dumps(e), case[3])
            if k not in seen:
                seen.add(k)
                yield e, ctx
    for img, D in GEOMETRIES:
        tr = T.Tracer(img, D)
        for rest in itertools.product(*REST):
            trace = json.loads(json.dumps(tr.trace(*rest)))
            ctx = _sched_ctx(tr, rest[0])
            for e in trace:
                k = (json.dumps(e), rest[0], img, D)
                if k not in seen:
                    seen.add(k)
                    yield e, ctx


def test_access_table_is_complete():
    """Every entry name of every traced case has a row (or is an ordering entry), and every argument is classified as a buffer
    or is a listed scalar: hazard_util.accesses raises Unclassified otherwise.  A new launch cannot slip past the checker."""
    names = set()
    for e, ctx in _all_entries():
        names.add(e[0])
        if e[0] in H.ORDERING:
            assert all(isinstance(v, list) or H.is_scalar(v) for v in e[1:]), e
            continue
        assert e[0] in H.ACCESS or e[0] in H.SPECIAL, "%r has no row in hazard_util.ACCESS" % (e,)
        stream, accs = H.accesses(e, ctx)
        assert stream in H.STREAMS, e
        assert accs or e[0] == "hook", "%r touches nothing" % (e,)
    assert not (set(H.ACCESS) - names), "rows for entries no case issues: %s" % sorted(set(H.ACCESS) - names)
    ctx = H.Context()
    for bad in (["dvae_new_kernel", "a", "b", "main"],                          # no row
                ["scale_", "a", "some_buffer", "main"],                         # a string where the row says scalar
                ["scale_", "B", 0.5, "main"],                                   # a scalar where the row says buffer
                ["copy_flat_", "a", "b", 3, "main"],                            # an argument more than the row
                ["dvae_fc_chain_fwd", ["FcChainFwdArgs", ["new_field", "a"]], "main"],
                ["dvae_linear_wgrad_grouped", [["x", "dy", "dw", "db", "B", "oops", 256]], 1, "main"]):
        with pytest.raises(H.Unclassified):
            H.accesses(bad, ctx)


def test_access_table_follows_the_header():
    """include/dvae_hip.h decides: a `const T*` parameter is read, a `T*` written (or both), anything else is no buffer."""
    protos = H.header_prototypes()
    for name, row in H.ACCESS.items():
        if not name.startswith("dvae_"):
            continue
        params = protos[name]
        assert len(params) == len(row), (name, params, row)
        for i, ((is_ptr, is_const), mode) in enumerate(zip(params, row)):
            want = (H.R,) if is_const else (H.W, H.RW)
            assert (mode in want) if is_ptr else mode is None, "%s argument %d: %r, the header says %s" % (
                name, i, mode, ("const pointer" if is_const else "pointer") if is_ptr else "no pointer")
    for struct, table in (("dvae_fc_chain_fwd_args", H.FC_FWD), ("dvae_fc_chain_bwd_args", H.FC_BWD)):
        fields = H.header_struct_fields(struct)
        assert set(fields) == set(table), (struct, set(fields) ^ set(table))
        # a `const` field the launch writes when the fused 4x4 ends ride along is listed in FC_*_ENDS, not here
        for k, (ptr, const) in fields.items():
            assert table[k] == ((H.R if const else H.W) if ptr else None), (struct, k)


def test_access_table_covers_the_step_invariants_tables():
    """test_step_schedule's WRITES / FC_FWD / FC_BWD were the starting point: what they call written is written here too
    (but for the two arguments that the header and csrc/capi.hip declare const)."""
    for name, positions in TS.WRITES.items():
        if name in H.ACCESS:
            for i in positions:
                assert H.ACCESS[name][i] in (H.W, H.RW) or (name, i) in H.CONST_IN_HEADER, (name, i)
    assert all(H.FC_FWD[k] == H.W for k in TS.FC_FWD if k != "kl_dim") and H.FC_FWD["kl_part"] == H.W
    assert all(H.FC_BWD[k] == H.W for k in TS.FC_BWD)
    assert set(TS.ORDERING) == set(H.ORDERING)


# ---- the exemptions ----------------------------------------------------------------------------------------------------------
def test_exemptions_are_few_and_hit():
    assert len(EXEMPT) <= MAX_EXEMPT
    for (first, second, buf), reason in EXEMPT.items():
        assert "_ws" not in buf and not buf.startswith(("g:", "dg:")), "no exemption on a workspace or a gradient: %s" % buf
        assert reason.strip().endswith(".") and ":" in reason, "one sentence with the file and line: %r" % reason
    if not EXEMPT:
        return
    hit = set()
    for model in MODELS:
        tracer = S.StepTracer(*model)
        for _, case in TS._cases_of(model):
            for _, trace in _step_traces(tracer, case):
                _hazards(trace, _step_ctx(tracer, case), hit)
    for img, D in GEOMETRIES:
        tracer = T.Tracer(img, D)
        for rest in itertools.product(*REST):
            traces = list(_sched_traces(tracer, rest))
            for _, trace in traces:
                _hazards(trace, _sched_ctx(tracer, rest[0]), hit)
    assert hit == set(EXEMPT), "stale exemptions: %s" % sorted(set(EXEMPT) - hit)


# ---- the checker on synthetic traces ---------------------------------------------------------------------------------------------
FORK, FORK2, JOIN = ["dvae_stream_order", "main", "side"], ["dvae_stream_order", "main", "wg2"], ["dvae_stream_order", "side", "main"]
WGRAD = lambda x, dy, dw, ws, stream: ["dvae_linear_wgrad", x, dy, dw, None, 16, 8, 8, ws, stream]
G_ALL = ["grads", "all"]
# name -> (the trace, the position of the edge that orders it, what is reported without that edge: kind, earlier, later, buffer
# -- positions in the trace WITHOUT the edge)
SYNTHETIC = {
    "a missing fork": ([["copy_flat_", "act", "src", "main"], FORK, WGRAD("act", "dy", "dw", "_ws_side", "side")],
                       1, ("RAW", 0, 1, "act")),
    "a missing join": ([FORK, WGRAD("act", "dy", "dw", "_ws_side", "side"), JOIN, ["host_read", "dw", "main"]],
                       2, ("RAW", 1, 2, "dw")),
    "a main-stream overwrite of a side-stream operand": (
        [["copy_flat_", "act", "src", "main"], FORK, WGRAD("act", "dy", "dw", "_ws_side", "side"), JOIN,
         ["copy_flat_", "act", "src2", "main"]], 3, ("WAR", 2, 3, "act")),
    "two streams on one workspace": (
        [FORK, WGRAD("a1", "dy1", "dw1", "_ws", "side"), JOIN, WGRAD("a2", "dy2", "dw2", "_ws", "main")],
        2, ("WAW", 1, 2, "_ws")),
    "an asynchronous all-reduce read before its wait": (
        [["copy_flat_", "grads", "src", "main"], ["all_reduce_async", G_ALL, "main"], ["wait", G_ALL, "main"],
         ["host_read", "grads", "main"]], 2, ("RAW", 1, 2, "grads")),
    "a side -> wg2 read with only main -> side and main -> wg2 edges": (
        [FORK, FORK2, ["copy_flat_", "t", "src", "side"], ["dvae_stream_order", "side", "wg2"],
         WGRAD("t", "dy", "dw", "_ws_wg2", "wg2")], 3, ("RAW", 2, 3, "t")),
}


@pytest.mark.parametrize("name", list(SYNTHETIC))
def test_checker_on_synthetic_traces(name):
    trace, edge, (kind, i, j, buf) = SYNTHETIC[name]
    ctx = H.Context()
    assert H.check(trace, ctx) == [], H.describe(name + ", with its edge", trace, H.check(trace, ctx))
    broken = trace[:edge] + trace[edge + 1:]
    assert H.check(broken, ctx) == [H.Hazard(kind, i, j, buf)], H.describe(name, broken, H.check(broken, ctx))
    text = H.describe(name, broken, H.check(broken, ctx))
    assert "%s on %s: entry %d is not ordered behind entry %d" % (kind, buf, j, i) in text and str(broken[j]) in text


def test_checker_knows_extents():
    """Disjoint slices of one arena, disjoint row ranges of one buffer and a collective's span do not conflict; overlapping ones do."""
    class Arena:
        offsets = {"a.weight": (0, 100), "a.bias": (100, 4), "b.weight": (104, 50)}
    ctx = H.Context({"g:": Arena}, {"B": 4, "Bh": 2, "D": 10})
    side = lambda dw, db: ["dvae_linear_wgrad", "x", "dy", dw, db, 16, 8, 8, "_ws_side", "side"]
    assert H.check([FORK, side("g:a.weight", "g:a.bias"), ["all_reduce", ["g:b.weight", 50], "main"]], ctx) == []
    assert H.check([FORK, side("g:a.weight", "g:a.bias"), ["all_reduce", ["g:a.bias", 54], "main"]], ctx) == [H.Hazard("WAW", 1, 2, "g:")]
    assert H.check([FORK, side("g:b.weight", None), ["optim.step", "vae", "main"]], ctx) == [H.Hazard("RAW", 1, 2, "g:")]
    halves = [FORK, ["dvae_permute_dims", "z+1BhD", "perm", "out", "Bh", 10, "side"], ["dvae_reparam_kl_fwd", "ml", None, "mu",
              "logvar", "z", None, None, "Bh", 10, "main"]]
    assert H.check(halves, ctx) == []
    halves[2][8] = "2Bh"
    assert H.check(halves, ctx) == [H.Hazard("WAR", 1, 2, "z")]


# ---- seeded faults: real traces with one ordering entry filtered out ------------------------------------------------------------
_M64 = ((3, 64, 64), 10)


def _first(trace, entry, after=None):
    lo = 0 if after is None else next(i for i, e in enumerate(trace) if e[0] == after)
    return next(i for i in range(lo, len(trace)) if trace[i] == entry)


def _last(trace, entry):
    return max(i for i, e in enumerate(trace) if e == entry)


# (what is dropped, the case, how to find it in the trace, the stream whose launch must be reported as the LATER entry)
SEEDED = [
    ("the backward pass's first fork", ("betaH", "train", _M64, 129, "float32", (1, 0), "global", "drawn", "default"),
     lambda t: _first(t, FORK), "side"),
    ("the wg2 fork", ("factor", "train", _M64, 2048, "float32", (1, 0), "global", "drawn", "default"),
     lambda t: _first(t, FORK2), "wg2"),
    ("the late join's event wait", ("btcvae", "train", _M64, 129, "float32", (1, 0), "global", "drawn", "default"),
     lambda t: _first(t, ["dvae_event_wait", "slot", "main"]), "main"),
    ("the final side -> main join", ("betaH", "train", _M64, 129, "float32", (1, 0), "global", "drawn", "default"),
     lambda t: _last(t, JOIN), "main"),
    ("the sharded exchange's wait", ("factor", "train", _M64, 128, "float32", (2, 0), "global", "drawn", "default"),
     lambda t: next(i for i, e in enumerate(t) if e[0] == "wait"), "main"),
    ("the sharded late join's side -> aux edge", ("btcvae", "train", _M64, 129, "float32", (2, 1), "global", "drawn", "default"),
     lambda t: _first(t, ["dvae_stream_order", "side", "aux"]), "aux"),
    ("the fork behind the FC chain", ("betaH", "train", ((1, 32, 32), 17), 129, "uint8", (1, 0), "global", "drawn", "default"),
     lambda t: _first(t, FORK, after="dvae_reparam_kl_bwd"), "side"),
]


def test_seeded_faults_are_found():
    """Drop ONE ordering call from a real step (the recorded list is filtered, the engine untouched): the checker must fail, on
    the stream that lost its edge.  A dropped edge that another path makes redundant is counted, not failed: at most 2."""
    redundant, tracers = [], {}
    for what, case, find, later in SEEDED:
        tracer = tracers.get(case[2]) or tracers.setdefault(case[2], S.StepTracer(*case[2]))
        ctx = _step_ctx(tracer, case)
        one = json.loads(json.dumps(tracer.trace(*(case[:2] + case[3:]))))
        two = lambda t: t + H.between_steps(t, True, case[0] == "factor") + t
        assert _hazards(two(one), ctx) == [], what
        k = find(one)
        assert one[k][0] in H.ORDERING, (what, one[k])
        cut = two(one[:k] + one[k + 1:])
        found = _hazards(cut, ctx)
        if not found:
            redundant.append(what)
            continue
        streams = {H.accesses(cut[h.j], ctx)[0] if cut[h.j][0] != "all_reduce_async" else "comm" for h in found}
        assert later in streams, H.describe("%s dropped (%s)" % (what, TS._label(case)), cut, found)
    assert len(redundant) <= 2 and len(SEEDED) - len(redundant) >= 5, "redundant edges: %s" % redundant
