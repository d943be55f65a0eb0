"""CPU: everything ONE native training (or evaluation) step issues -- ``loss_f.fused_step`` / ``FactorKLoss.call_optimize``,
from ``engine.stage`` to the final join or all-reduce -- recorded without a GPU and without libdvae_hip.so.

schedule_trace.py records the engine's backward pass; this is the code that calls the engine (models/losses.py): forward,
estimator fork, loss epilogue, late join, sharded exchanges, gradient all-reduce.  On top of schedule_trace.recording:

  * ``call`` / ``_stream`` of models.losses and models.discriminator are the recorder and the current stream NAME;
    ``torch.cuda.stream`` / ``torch.cuda.current_stream`` work over the same names ("main", "side", "aux", "wg2");
  * ``losses.scale_`` / ``copy_flat_`` / ``record_py`` are recorders (["scale_", ...], ["copy_flat_", ...], ["py", ...]);
  * a fake communicator records every collective with its buffer and the stream it was issued on;
  * ``knob`` answers from the case's switches; ``optim.step`` and ``assign_grads`` do nothing; replay is off;
  * host argument structs (FC chains, the staging launch) are recorded by content instead of by address.

Pointers read as buffer names; a pointer INTO a buffer as ``name+kBD`` (k x rows x latent_dim elements; ``Bh`` = half batch
for FactorVAE) or ``name+elements``.  Row counts are symbols (``B``, ``WB`` = world x B, ``Bh``, ``2Bh``), each after a
check that the argument IS that quantity; KL block counts read ``klb(rows)`` (the stand-in library works 8 rows per block);
the event slot reads ``slot``.

tests/test_step_schedule.py compares these traces with tests/golden/step_launch_trace.json.  To print one (loss, mode,
geometry, latent_dim, rows, dtype, world, rank, estimator, noise, switch):

  python tests/step_trace.py btcvae train 3,64,64 10 128 float32 2 0 global drawn DVAE_LATE_JOIN=0
"""
import bisect
import contextlib
import ctypes
import itertools
import os
import sys
from unittest import mock

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import schedule_trace as T  # noqa: E402  (also puts the package on sys.path)

import torch  # noqa: E402

from disvae_amd import _lib, engine as E, optim, schedule as SCHED  # noqa: E402
from disvae_amd.models import discriminator as DISC, losses as L, vae as V  # noqa: E402

# ---- the cases ---------------------------------------------------------------------------------------------------------
# one switch at a time against the default: the knob values schedule.build_policy is given
SWITCHES = {
    "default": {},
    "DVAE_STREAMS=1": {"DVAE_STREAMS": "1"},
    "DVAE_LATE_JOIN=0": {"DVAE_LATE_JOIN": "0"},
    "SMALL_SHARD_ELEMS=0": {"DVAE_SMALL_SHARD_ELEMS": "0"},             # the two-span gradient exchange
    "DVAE_DISC_WGRAD_SIDE=0": {"DVAE_DISC_WGRAD_SIDE": "0"},
    "DVAE_DISC_CHAIN2_AUX=1": {"DVAE_DISC_CHAIN2_AUX": "1"},
    "DVAE_FORK_HOOK=0": {"DVAE_FORK_HOOK": "0"},
    "eager_wgrad": {"DVAE_EAGER_WGRAD_ELEMS": str(1 << 40)},
    "DVAE_TAIL_MAIN=": {"DVAE_TAIL_MAIN": ""},
}
AXES = {
    "loss": ["betaH", "betaB", "btcvae", "factor"],
    "mode": ["train", "eval"],
    # (geometry, latent_dim): thinned from the 2 x 2 product -- the tuned geometry with the fused FC chain, the small one with per-layer FC launches
    "model": [((3, 64, 64), 10), ((1, 32, 32), 17)],
    # thinned: 128 / 2048 for FactorVAE (even; both sides of its THREE_STREAM_MIN_ROWS), 129 (odd) for the others -- no other row
    # threshold acts on the step outside the engine's backward pass with replay off, and those are schedule_trace's business
    "rows": [128, 129, 2048],
    "dtype": ["float32", "uint8"],
    "world": [(1, 0), (2, 0), (2, 1)],
    "estimator": ["global", "local"],
    "noise": ["drawn", "injected"],
    "switch": list(SWITCHES),
}


def dropped(loss, mode, model, rows, dtype, world, estimator, noise, switch):
    """Why a combination of AXES is not a case (None: it is one)."""
    if loss == "factor" and rows % 2:
        return "FactorVAE splits the batch in two halves: even rows only"
    if loss != "factor" and rows != 129:
        return "thinned: one (odd) row count for the single-optimizer losses, whose step has no row threshold of its own"
    if estimator == "local" and (world[0] == 1 or loss not in ("btcvae", "factor")):
        return "the estimator's scope exists only for the batch-coupled losses under data parallelism"
    if switch.startswith("DVAE_DISC_") and loss != "factor":
        return "a discriminator switch, read by FactorVAE's step only"
    if switch == "SMALL_SHARD_ELEMS=0" and world[0] == 1:
        return "the gradient exchange exists only under data parallelism"
    if switch != "default" and (dtype == "uint8" or noise == "injected"):
        return "thinned: uint8 input and injected noise are crossed with the default switches only (no switch reads either)"
    if mode == "eval" and noise == "injected":
        return "evaluation draws no noise"
    if mode == "eval" and switch not in ("default", "DVAE_STREAMS=1"):
        return "the switch acts on the backward pass / the late join, which evaluation does not have"
    if mode == "eval" and dtype == "uint8" and rows == 2048:
        return "thinned: evaluation's uint8 input path does not depend on the row count"
    return None


def cases():
    return (c for c in itertools.product(*AXES.values()) if dropped(*c) is None)


# entry point -> positions of its row-count arguments
ROW_ARGS = {
    "dvae_conv32_down": (6,), "dvae_conv32_up": (6,), "dvae_conv32_up_bits": (6,), "dvae_convT3_dgrad_bits": (4,),
    "dvae_convT4s2_dgrad": (6,), "dvae_linear_dgrad": (5,), "dvae_convT4s2_wgrad": (6,), "dvae_conv4s2_wgrad": (6,),
    "dvae_conv4s2_wgrad_u8": (4,), "dvae_conv1_fwd_bits": (6,), "dvae_conv4s2_fwd_u8": (4,), "dvae_conv4s2_fwd": (6,),
    "dvae_linear_fwd": (4,), "dvae_reparam_kl_fwd": (7,), "dvae_reparam_kl_bwd": (11,), "dvae_convT3_fwd_staged": (10,),
    "dvae_convT4s2_sigmoid_recon_fwd_u8": (9,), "dvae_convT4s2_sigmoid_recon_fwd": (10,), "dvae_loss_epilogue": (6, 8),
    "dvae_loss_finalize": (3,), "dvae_loss_pack": (4,), "dvae_btcvae_fwd": (3, 5, 6), "dvae_btcvae_bwd": (4, 6, 7),
    "dvae_permute_dims": (3,), "dvae_disc_losses": (1,), "dvae_linear_wgrad": (4,), "all_reduce_cols_sums": (1,),
}
KLB_ARGS = {"dvae_loss_epilogue": 3, "dvae_kl_finish": 1}
ROW_FIELDS = ("n_enc", "n_kl", "n_dec", "n")      # of the FC chains' argument structs
KLB_ROWS = 8                                       # the stand-in library's dvae_fc_chain_rows


class _Lib(T._Lib):
    @staticmethod
    def dvae_fc_chain_rows(n):
        return KLB_ROWS


class _CudaFace:
    """The discriminator's parameter arena with a `flat` that says it lives on a GPU (forward_raw refuses CPU arenas)."""

    class _Dev:
        type = "cuda"

        def __eq__(self, other):
            return True

        def __ne__(self, other):
            return False

    class _Flat:
        def __init__(self, t):
            self._t, self.device = t, _CudaFace._Dev()

        def __getattr__(self, k):
            return getattr(self._t, k)

    def __init__(self, arena):
        self._arena, self.flat = arena, _CudaFace._Flat(arena.flat)

    def __getattr__(self, k):
        return getattr(self._arena, k)


class FakeComm:
    """world_size / rank and the collectives the loss plugins call, as trace entries."""

    def __init__(self, tracer, world, rank):
        self.tr, self.world_size, self.rank, self._bufs = tracer, world, rank, {}

    def _buf(self, name, shape):
        b = self._bufs.get((name, shape))
        if b is None:
            b = self._bufs[(name, shape)] = torch.empty(shape)
        return b

    def _rec(self, what, *args):
        self.tr.out.append((what,) + args + (self.tr.stream(),))

    def all_reduce(self, t):
        self._rec("all_reduce", ("span", t.data_ptr(), t.numel()))
        return t

    def all_reduce_async(self, t):
        span, tr = ("span", t.data_ptr(), t.numel()), self
        self._rec("all_reduce_async", span)

        class _Handle:
            def wait(self):
                tr._rec("wait", span)
        return _Handle()

    def all_reduce_cols_sums(self, xbuf, B, D, n_tail):
        self._rec("all_reduce_cols_sums", ("span", xbuf.data_ptr(), xbuf.numel()), B, D, n_tail)
        return xbuf

    def all_gather_latents(self, z, mu, logvar):
        B, D = z.shape
        glob = self._buf("lat_glob", (3, self.world_size * B, D))
        self._rec("all_gather_latents", z.data_ptr(), mu.data_ptr(), logvar.data_ptr(), glob.data_ptr())
        return glob[0], glob[1], glob[2]

    def all_gather_rows(self, t, name="rows"):
        out = self._buf("rows_glob", (self.world_size * t.shape[0],) + tuple(t.shape[1:]))
        self._rec("all_gather_rows", t.data_ptr(), out.data_ptr())
        return out


class StepTracer:
    """One CPU model of (img, D) with its engine and one loss object per loss; trace() runs one step."""

    def __init__(self, img, D):
        self.img, self.D = tuple(img), D
        self.out, self.streams, self.knobs = [], ["main"], {}
        with self.recording():
            self.model = V.init_specific_model("Burgess", img, D)
            self.eng = self.model._engine = E.VAEEngine(self.model.img_size, D, self.model.arena)
            self.eng.images
            self.losses = {"betaH": L.BetaHLoss(), "betaB": L.BetaBLoss(), "btcvae": L.BtcvaeLoss(n_data=1000),
                           "factor": L.FactorKLoss("cpu", disc_kwargs=dict(latent_dim=D))}
        for f in self.losses.values():
            f.replay = None
        disc = self.losses["factor"].discriminator
        self.disc_arena = disc._arena
        self.noise = {}

    # ---- the patches ----------------------------------------------------------------------------------------------------
    def stream(self):
        return self.streams[-1]

    @contextlib.contextmanager
    def _on(self, st):
        self.streams.append(st.cuda_stream)
        try:
            yield
        finally:
            self.streams.pop()

    def _call(self, name, *args):
        if name == "dvae_stage_weights":     # host tables by content: (convs, FCs, thin layer?, coef, the coefficients, stream)
            im = self.eng.images
            args = (args[1], args[3], args[4] is not None, args[5], None if args[6] is None else tuple(im.coef_vals), args[7])
        self.out.append((name,) + args)

    def _py(self, fn, *args):
        self.out.append(("py", fn.__name__, fn.__self__.data_ptr()) + tuple(a.data_ptr() for a in args) + (self.stream(),))
        return fn(*args)

    @contextlib.contextmanager
    def recording(self):
        with contextlib.ExitStack() as st:
            st.enter_context(T.recording(self.out))
            p = lambda obj, name, new: st.enter_context(mock.patch.object(obj, name, new))
            p(_lib, "lib", lambda: _Lib)
            p(_lib, "struct_of", lambda cls, **kw: (None, ("args", cls.__name__) + tuple(sorted(kw.items()))))
            for mod in (E, L, DISC):
                p(mod, "call", self._call)
                p(mod, "_stream", self.stream)
            for mod in (E, L, SCHED):
                p(mod, "knob", lambda name, default: self.knobs.get(name, default))
            p(SCHED, "enabled", lambda: True)            # (the switches are read afresh for every step)
            p(torch.cuda, "stream", self._on)
            p(torch.cuda, "current_stream", lambda *a: T._Stream(self.stream()))
            p(L, "scale_", lambda t, alpha: self.out.append(("scale_", t.data_ptr(), alpha, self.stream())))
            p(L, "copy_flat_", lambda o, s_: self.out.append(("copy_flat_", o.data_ptr(), s_.data_ptr(), self.stream())))
            p(L, "record_py", self._py)
            p(optim, "step", lambda optimizer: None)
            p(V.VAE, "engine", property(lambda m: m._engine))
            p(V.VAE, "assign_grads", lambda m: None)
            p(DISC.Discriminator, "assign_grads", lambda d: None)
            yield

    # ---- names ------------------------------------------------------------------------------------------------------------
    def _names(self, loss_f, x, injected):
        exact, spans = {}, []

        def add(name, t):
            if isinstance(t, torch.Tensor):
                exact.setdefault(t.data_ptr(), name)
                spans.append((t.data_ptr(), t.numel() * t.element_size(), name))

        def add_fields(prefix, d):
            for field, v in d.items():
                if isinstance(v, list):
                    for i, t in enumerate(v):
                        add("%s%s[%d]" % (prefix, field, i), t)
                elif field != "lat3":
                    add(prefix + field, v)
        eng, disc = self.eng, getattr(loss_f, "discriminator", None)
        for buf in eng._bufs.values():
            add_fields("", vars(buf))
        for k in eng.arena.shapes:
            add("p:" + k, eng.p(k))
            add("g:" + k, eng.g(k))
        for (layer, kind), p_ in eng.images.ptrs.items():
            exact[p_] = "img:%s:%s" % (layer, kind)
        for ws in ("_ws", "_ws_side", "_ws_wg2"):
            add(ws, getattr(eng, ws))
        add("x", x)
        sc = loss_f._scratch
        add_fields("", {k: v for k, v in vars(sc).items() if k != "lat"})
        for (name, _, _), t in sc.lat.items():
            add(name, t)
        for (name, _, _), t in loss_f._static.items():
            add("static:" + name, t)
        for name, t in injected.items():
            add(name, t)
        if loss_f.comm is not None:
            for (name, _), t in loss_f.comm._bufs.items():
                add(name, t)
        if disc is not None:
            for k in self.disc_arena.shapes:
                add("dp:" + k, self.disc_arena.view(k))
                add("dg:" + k, self.disc_arena.view(k, grad=True))
            for acts in disc._acts.values():
                add_fields("disc.", acts)
            for ws in ("_wsbuf", "_wsbuf_side", "_wsbuf_aux"):
                add("disc." + ws, getattr(disc, ws, None))
        spans.sort()
        return exact, spans

    def _name(self, v):
        if isinstance(v, tuple):
            if v and v[0] == "span":         # a collective's buffer: [name, elements or "all" (= the whole named buffer)]
                base, nbytes, _ = self._span(v[1])
                return [self._name(v[1]), "all" if (v[1] == base and v[2] * 4 == nbytes) else v[2]]
            return [self._name(u) for u in v]
        if not (isinstance(v, int) and not isinstance(v, bool) and v >= 1 << 32):
            return v
        if v in self.exact:
            return self.exact[v]
        base, _, name = self._span(v)
        off = (v - base) // 4
        k, r = divmod(off, self.unit[1] * self.D)
        return "%s+%d%sD" % (name, k, self.unit[0]) if r == 0 else "%s+%d" % (name, off)

    def _span(self, p_):
        i = bisect.bisect_right(self.spans, (p_, 1 << 62, "")) - 1
        if i < 0 or not (self.spans[i][0] <= p_ < self.spans[i][0] + self.spans[i][1]):
            raise KeyError("a pointer into no buffer of the step: %#x" % p_)
        return self.spans[i]

    def _sym(self, v, ent):
        if v in (0, 1):                   # no rows / dvae_loss_epilogue's denominator when it only packs
            return v
        for name, val in self.rows:
            if v == val:
                return name
        raise AssertionError("%r: %r is none of the step's row counts %r" % (ent, v, self.rows))

    def _klb(self, v, ent):
        if v == 0:
            return 0
        for name, val in self.rows:
            if v == (val + KLB_ROWS - 1) // KLB_ROWS:
                return "klb(%s)" % name
        raise AssertionError("%r: %r is the KL block count of none of %r" % (ent, v, self.rows))

    def _entry(self, raw, loss_f, x):
        ent = self._name(raw)
        name = ent[0]
        for i in ROW_ARGS.get(name, ()):
            ent[i + 1] = self._sym(ent[i + 1], raw)
        if name in KLB_ARGS:
            ent[KLB_ARGS[name] + 1] = self._klb(ent[KLB_ARGS[name] + 1], raw)
        if name in ("dvae_event_record", "dvae_event_wait"):
            assert ent[1] == loss_f._ev_slot, raw
            ent[1] = "slot"
        elif name == "dvae_u8_to_f32":
            assert ent[3] == x.numel(), raw
            ent[3] = "numel(x)"
        elif name == "dvae_stage_weights" and ent[5] is not None:
            inv_b = 1.0 / (self.unit[1] * self.world)
            assert ent[5][_lib.C_INV_B] == ctypes.c_float(inv_b).value, (raw, inv_b)
            ent[5][_lib.C_INV_B] = "1/(W%s)" % self.unit[0]
        elif name == T.GROUPED:
            for prob in ent[1][1:]:
                prob[4] = self._sym(prob[4], raw)
            ent[1] = ent[1][1:]
        elif name in ("dvae_fc_chain_fwd", "dvae_fc_chain_bwd"):
            for kv in ent[1][2:]:
                if kv[0] in ROW_FIELDS:
                    kv[1] = self._sym(kv[1], raw)
            # (a field that points at the buffer of its own name -- most do -- is left out)
            ent[1] = ent[1][1:2] + [kv for kv in ent[1][2:] if kv[0] != kv[1]]
        return ent

    # ---- one step ---------------------------------------------------------------------------------------------------------
    def trace(self, loss, mode, rows, dtype, world, estimator, noise, switch):
        eng, model, loss_f, D = self.eng, self.model, self.losses[loss], self.D
        W, rank = world
        B, Bh = rows, rows // 2
        factor = loss == "factor"
        self.world = W
        self.unit = ("Bh", Bh) if factor else ("B", B)
        self.rows = [("Bh", Bh), ("2Bh", 2 * Bh), ("WBh", W * Bh)] if factor else [("B", B), ("WB", W * B)]
        eng._fc_descs.clear()
        self.knobs = SWITCHES[switch]
        loss_f.comm = FakeComm(self, W, rank) if W > 1 else None
        loss_f.estimator = estimator
        model.training = mode == "train"
        x = torch.empty((B,) + self.img, dtype=getattr(torch, dtype))
        f = lambda *s: torch.empty(*s)
        ew = W if (W > 1 and estimator == "global") else 1
        perms = torch.zeros(D, max(Bh * ew, 1), dtype=torch.int64)
        injected = {}
        if noise == "injected":
            injected = ({"eps1_in": f(Bh, D), "eps2_in": f(Bh, D), "perms_in": perms} if factor else {"eps_in": f(B, D)})
        del self.out[:], self.streams[1:]
        with self.recording():
            if factor:
                disc = loss_f.discriminator
                disc._arena = self.disc_arena         # its workspaces are allocated on the real (CPU) arena's device ...
                disc._act_buffers(2 * Bh), disc._act_buffers(Bh)
                for side in (False, True, "aux"):
                    disc._ws(side)
                disc._arena = _CudaFace(self.disc_arena)   # ... and the step sees an arena that claims a GPU
                loss_f._draw_perms = lambda D_, n: (perms, None)      # (the pinned staging ring needs a device)
                loss_f.call_optimize(x, model, None, None, noise=tuple(injected.values()) or None)
            else:
                loss_f.fused_step(x, model, None, None, eps=injected.get("eps_in"))
        assert self.streams == ["main"]
        self.exact, self.spans = self._names(loss_f, x, injected)
        trace = [self._entry(raw, loss_f, x) for raw in self.out]
        if rows >= 1024:                             # the workspaces of a large step: not kept
            eng._bufs.clear()
            loss_f._scratch.lat.clear()
            loss_f._static.clear()
            if factor:
                loss_f.discriminator._acts.clear()
        return trace


def all_traces():
    """(case, trace) for every case, in the order of cases()."""
    tracers = {}
    for case in cases():
        loss, mode, (img, D), rows, dtype, world, estimator, noise, switch = case
        tr = tracers.get((img, D))
        if tr is None:
            tr = tracers[(img, D)] = StepTracer(img, D)
        yield case, tr.trace(loss, mode, rows, dtype, world, estimator, noise, switch)


def pack(commit):
    """The fixture, packed like backward_launch_trace.json -- distinct entries once, distinct traces once, one index per case --
    with one level more, or it would not fit the size allowed to a committed fixture: a trace is a list of RUNS, a run the
    entries up to and including a dvae_stream_order (steps that differ in one switch share most of their runs)."""
    import json
    entries, runs, traces, idx = {}, {}, {}, []
    for _, trace in all_traces():
        t, run = [], []
        for e in trace:
            run.append(entries.setdefault(json.dumps(e), len(entries)))
            if e[0] == "dvae_stream_order":
                t.append(runs.setdefault(tuple(run), len(runs)))
                run = []
        if run:
            t.append(runs.setdefault(tuple(run), len(runs)))
        idx.append(traces.setdefault(tuple(t), len(traces)))
    return {"generated_from": commit, "axes": json.loads(json.dumps(AXES)), "entries": [json.loads(e) for e in entries],
            "runs": [list(r) for r in runs], "traces": [list(t) for t in traces], "cases": idx}


def unpack(fx, i):
    """The recorded trace of case number i of a packed fixture."""
    return [fx["entries"][e] for r in fx["traces"][fx["cases"][i]] for e in fx["runs"][r]]


if __name__ == "__main__":
    if sys.argv[1] == "--write":            # --write <file> <commit the loss plugins are at>: the fixture (recorded ONCE, from
        import json                         # the commit before models/losses.py was reorganised; not regenerated since)
        with open(sys.argv[2], "w") as f:
            json.dump(pack(sys.argv[3]), f, separators=(",", ":"))
        sys.exit(0)
    loss, mode, img, D, rows, dtype, W, rank, estimator, noise = sys.argv[1:11]
    switch = sys.argv[11] if len(sys.argv) > 11 else "default"
    case = (loss, mode, (tuple(int(v) for v in img.split(",")), int(D)), int(rows), dtype, (int(W), int(rank)), estimator,
            noise, switch)
    if dropped(*case):
        sys.exit("not a case: " + dropped(*case))
    for e in StepTracer(case[2][0], int(D)).trace(loss, mode, int(rows), dtype, (int(W), int(rank)), estimator, noise, switch):
        print(e)
