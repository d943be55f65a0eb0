"""CPU: the launch sequence of VAEEngine's backward pass, recorded without a GPU and without libdvae_hip.so.

A VAEEngine is host-side state only: with ``engine.call`` replaced by a recorder, the streams by names ("main", "side",
"wg2", "aux") and every pointer argument translated back to the name of the buffer it points into, one backward pass reads
as a list of entries such as

  ['dvae_convT4s2_wgrad', 'dec_act[2]', 1, 'g_logit', 0, 'g:decoder.convT3.weight', 'g:decoder.convT3.bias', 'B', 32,
   32, 32, 3, '_ws_side', 'side']

(the row count is written 'B' -- after a check that it IS the step's row count -- so that steps of different sizes that
are scheduled alike share one trace).  The grouped FC weight-gradient launch records its problem list in place of the
host address of its descriptor array; ``fc_chain`` and the ``at_next_fork`` hook are markers.

The whole step around the backward pass (forward, loss epilogue, exchanges: models/losses.py) is tests/step_trace.py's.

tests/test_backward_schedule.py compares these traces with tests/golden/backward_launch_trace.json.  To print one:

  python tests/schedule_trace.py 3,64,64 10 1024 default float32 step
"""
import contextlib
import itertools
import os
import sys
from unittest import mock

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "disentangling-vae_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

from disvae_amd import _lib, engine as E, schedule as SCHED  # noqa: E402
from disvae_amd.models.vae import init_specific_model  # noqa: E402

# ---- the cases: the cross product of AXES, in this order ---------------------------------------------------------------
AXES = {
    "geometry": [(3, 64, 64), (1, 64, 64), (1, 32, 32)],
    "latent_dim": [10, 17],                  # 17: per-layer FC launches, fuse_ends off
    # both sides of every row threshold of disvae_amd/schedule.py: EARLY_THIN_2_ROWS 112-128, FCW_MAIN_ROWS 129-320,
    # FUSE_ENDS_MAX_ROWS 256, THREE_STREAM_MIN_ROWS_FACTOR 2048
    "rows": [16, 112, 128, 129, 256, 257, 320, 321, 1024, 2048],
    "policy": ["default", "eager_wgrad", "single_stream", "three_streams", "sharded", "tail_main_none"],
    "dtype": ["float32", "uint8"],
    "calls": ["step", "step_nohook", "step_nodefer", "autograd", "autograd_hook", "decode", "encode"],
}
# what schedule.build_policy is given, per policy: (debug switches off their shipped value, world size)
POLICY = {"default": ({}, 1), "eager_wgrad": ({"DVAE_EAGER_WGRAD_ELEMS": str(1 << 40)}, 1),
          "single_stream": ({"DVAE_STREAMS": "1"}, 1), "three_streams": ({"DVAE_THREE_STREAM_MIN_ROWS": "0"}, 1),
          "sharded": ({}, 2), "tail_main_none": ({"DVAE_TAIL_MAIN": ""}, 1)}


def policy(img, D, B, name):
    """The StepPolicy of case (img, D, B, policy name)."""
    over, world = POLICY[name]
    return SCHED.build_policy(tuple(img), D, B, tuple(over.get(k, v) for k, v in SCHED.SWITCHES), world)


def cases():
    return itertools.product(*AXES.values())


# entry point -> (index of its row-count argument, index of the tensor it writes: None for a weight gradient)
ROWS_OUT = {
    "dvae_convT4s2_wgrad": (6, None), "dvae_conv4s2_wgrad": (6, None), "dvae_conv4s2_wgrad_u8": (4, None),
    "dvae_conv32_down": (6, 4), "dvae_conv32_up": (6, 5), "dvae_conv32_up_bits": (6, 4), "dvae_convT3_dgrad_bits": (4, 3),
    "dvae_convT4s2_dgrad": (6, 4), "dvae_linear_dgrad": (5, 4),
}
CONV_WGRADS = ("dvae_convT4s2_wgrad", "dvae_conv4s2_wgrad", "dvae_conv4s2_wgrad_u8")
GROUPED = "dvae_linear_wgrad_grouped"


class _Stream:
    def __init__(self, name):
        self.cuda_stream = name


class _Lib:
    @staticmethod
    def dvae_conv_wgrad_ws_floats():
        return 1024


@contextlib.contextmanager
def recording(out):
    """Inside: engines are built without the library, streams are names and every C-ABI call of engine.py lands in `out`."""
    with contextlib.ExitStack() as st:
        st.enter_context(mock.patch.object(_lib, "lib", lambda: _Lib))
        st.enter_context(mock.patch.object(_lib, "wgrad_descs", lambda problems: (None, ("descs",) + tuple(problems))))
        st.enter_context(mock.patch.object(E, "call", lambda name, *args: out.append((name,) + args)))
        st.enter_context(mock.patch.object(E, "_stream", lambda: "main"))
        st.enter_context(mock.patch.object(E, "wg2_stream", lambda device: _Stream("wg2")))
        st.enter_context(mock.patch.object(E, "device_streams", lambda device: (_Stream("side"), _Stream("aux"))))
        yield


class Tracer:
    """One engine over a CPU model of (img, D); trace() runs one backward pass and returns its launches."""

    def __init__(self, img, D):
        self.out = []
        with recording(self.out):
            m = init_specific_model("Burgess", img, D)
            self.eng = eng = E.VAEEngine(m.img_size, m.latent_dim, m.arena)
            # the schedule reads pointers and the row count it is given, never the workspace's size: one-row buffers stand in
            # for those of every batch size
            self.buf = buf = eng.buffers(1)
            images = eng.images
        self.img, self.D = tuple(img), D
        names = {}
        for field, v in vars(buf).items():
            if isinstance(v, list):
                for i, t in enumerate(v):
                    names[t.data_ptr()] = "%s[%d]" % (field, i)
            elif isinstance(v, torch.Tensor) and field != "lat3":       # (lat3 is z, mu, logvar in one allocation)
                names[v.data_ptr()] = field
        for k in eng.arena.shapes:
            names[eng.p(k).data_ptr()] = "p:" + k
            names[eng.g(k).data_ptr()] = "g:" + k
        for (layer, kind), p in images.ptrs.items():
            names[p] = "img:%s:%s" % (layer, kind)
        for ws in ("_ws", "_ws_side", "_ws_wg2"):
            names[getattr(eng, ws).data_ptr()] = ws
        self.x = {dt: torch.empty((1,) + self.img, dtype=getattr(torch, dt)) for dt in AXES["dtype"]}
        for t in self.x.values():
            names[t.data_ptr()] = "x"
        self.names = names

    def _name(self, v):
        if isinstance(v, tuple):
            return [self._name(u) for u in v]
        if isinstance(v, int) and not isinstance(v, bool) and v >= 1 << 32:
            return self.names[v]            # KeyError: a pointer into nothing the engine owns
        return v

    def _entry(self, raw, B):
        ent = self._name(raw)
        if ent[0] in ROWS_OUT:
            i = ROWS_OUT[ent[0]][0] + 1
            assert ent[i] == B, (ent, B)
            ent[i] = "B"
        elif ent[0] == GROUPED:
            for prob in ent[1][1:]:
                assert prob[4] == B, (ent, B)
                prob[4] = "B"
            ent[1] = ent[1][1:]
        return ent

    def trace(self, B, policy, dtype, calls):
        eng, buf, out = self.eng, self.buf, self.out
        eng.begin_step(globals()["policy"](self.img, self.D, B, policy))
        buf.B = B
        x = self.x[dtype].expand((B,) + self.img)
        z = buf.z.expand(B, self.D)
        del out[:]

        def fc_chain():      # as the loss plugins' (models/losses.py): a deferred epilogue must be forked before the chain
            eng.flush_fork_hook()
            out.append(("fc_chain",))
        with recording(out):
            if calls in ("step", "step_nodefer", "autograd_hook"):
                eng.at_next_fork(lambda: out.append(("hook",)))
            if calls in ("step", "step_nohook", "step_nodefer"):       # the native step of the loss plugins
                dec_fc = eng.decode_backward(z, buf, n=B, join=False, defer_fc_wgrad=calls != "step_nodefer", fc_chain=fc_chain)
                eng.encode_backward(x, buf, n=B, fc_chain=True, dec_fc=dec_fc)
            elif calls in ("autograd", "autograd_hook"):                # models/vae.py: _VAEFn.backward
                eng.encode_backward(x, buf, dec_fc=eng.decode_backward(z, buf, defer_fc_wgrad=True))
            elif calls == "decode":                                     # _DecodeFn.backward
                eng.decode_backward(z, buf)
            else:                                                       # _EncodeFn.backward
                assert calls == "encode", calls
                eng.encode_backward(x, buf)
        return [self._entry(raw, B) for raw in out]


def all_traces():
    """(case, trace) for every case of the cross product, in its order."""
    tracers = {}
    for case in cases():
        img, D, B, policy, dtype, calls = case
        tr = tracers.get((img, D))
        if tr is None:
            tr = tracers[(img, D)] = Tracer(img, D)
        yield case, tr.trace(B, policy, dtype, calls)


def pack(commit):
    """The fixture: every distinct entry once, every distinct trace once (as entry indices), one trace index per case."""
    import json
    entries, traces, idx = {}, {}, []
    for _, trace in all_traces():
        t = tuple(entries.setdefault(json.dumps(e), len(entries)) for e in trace)
        idx.append(traces.setdefault(t, len(traces)))
    return {"generated_from": commit, "axes": {k: [list(v) if isinstance(v, tuple) else v for v in vs] for k, vs in AXES.items()},
            "entries": [json.loads(e) for e in entries], "traces": [list(t) for t in traces], "cases": idx}


if __name__ == "__main__":
    if sys.argv[1] == "--write":            # --write <file> <commit the engine is at>: the fixture (recorded ONCE, from the
        import json                         # commit before the schedule code was reorganised; not regenerated since)
        with open(sys.argv[2], "w") as f:
            json.dump(pack(sys.argv[3]), f, separators=(",", ":"))
        sys.exit(0)
    img, D, B, policy, dtype, calls = sys.argv[1:7]
    for e in Tracer(tuple(int(v) for v in img.split(",")), int(D)).trace(int(B), policy, dtype, calls):
        print(e)
