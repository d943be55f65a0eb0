"""CPU: a happens-before checker for the traces of tests/step_trace.py and tests/schedule_trace.py.

The two trace fixtures pin WHAT a step issues; this states what must hold of any schedule.  Every entry of a trace is turned
into the buffer accesses it makes (ACCESS below: read, write or both, per argument position) and into the ordering it
creates; then

    two entries on DIFFERENT streams whose accesses CONFLICT -- the same base buffer, extents not known to be disjoint, at
    least one of the two a write -- must be ordered: the earlier one happens-before the later one.

Happens-before is program order within a stream plus the edges of the ordering entries:
  * dvae_stream_order(a, b): everything earlier on a -> everything later on b;
  * dvae_event_record(slot, a) ... dvae_event_wait(slot, b): what a held at the record -> everything later on b;
  * all_reduce_async(span) on a ... wait(span) on b: the collective runs on the communication stream ("comm") behind what a
    held when it was issued; what is behind the wait on b is behind the collective.  A blocking collective is a launch.
It is computed as one vector clock per stream (entry i on stream s with tick t happens-before entry j iff j's clock holds
clock[s] >= t): one pass over the trace, a constant-time question per pair of accesses.

A hazard reads RAW (the later entry reads what the earlier wrote), WAR (it overwrites what the earlier reads) or WAW.

Pointers are the names of the traces: ``name``, ``name+kBD`` / ``name+kBhD`` (k x rows x latent_dim elements) or
``name+elements``.  The slices of a parameter / gradient arena (``p:``, ``g:``, ``dp:``, ``dg:``) are extents of ONE base buffer
each, at their arena offsets, so that an all-reduce of a span and the launches that write into it meet.  Other extents come
from the entry's own arguments where EXTENT_ROWS gives them (rows x width), from the ("span", ptr, n) of a collective; an
access without a derivable extent is the whole buffer from its offset on.
"""
import os
import re
from collections import namedtuple

R, W, RW = "R", "W", "RW"
_ = None          # an argument that is not a buffer

# ---- what an entry touches: one letter per argument (the trailing stream excluded) ------------------------------------------
# C-ABI launches: include/dvae_hip.h -- a `const T*` is read, a `T*` written (test_access_table_follows_the_header compares);
# the in/out knowledge is the one of tests/test_gpu_memory_contract.py and tests/guard_util.py (workspaces are written by
# their launch; every optional pointer may be None in a trace and is then skipped)
ACCESS = {
    "dvae_conv1_fwd_bits": (R, _, R, R, W, W, _, _),
    "dvae_conv32_down": (R, R, R, R, W, _, _, _, _),
    "dvae_conv32_up": (R, _, R, R, R, W, _, _, _),
    "dvae_conv32_up_bits": (R, R, R, R, W, W, _, _),
    "dvae_convT3_fwd_staged": (R, R, R, R, _, W, W, _, R, W, _, _),
    "dvae_convT3_dgrad_bits": (R, R, R, W, _, _),
    "dvae_convT4s2_wgrad": (R, _, R, _, W, W, _, _, _, _, _, W),
    "dvae_conv4s2_wgrad": (R, _, R, _, W, W, _, _, _, _, _, W),
    "dvae_conv4s2_wgrad_u8": (R, R, W, W, _, _, _, _, _, W),
    "dvae_conv4s2_fwd": (R, _, R, R, W, _, _, _, _, _, _, _),
    "dvae_convT4s2_dgrad": (R, _, R, R, W, _, _, _, _, _, _),
    "dvae_convT4s2_sigmoid_recon_fwd": (R, _, R, R, R, W, W, _, R, W, _, _, _, _, _),
    "dvae_linear_fwd": (R, R, R, W, _, _, _, _, W),
    "dvae_linear_dgrad": (R, R, R, _, W, _, _, _, W),
    "dvae_linear_wgrad": (R, R, W, W, _, _, _, W),
    "dvae_reparam_kl_fwd": (R, R, W, W, W, W, R, _, _),
    "dvae_reparam_kl_bwd": (R, R, R, R, R, R, R, R, R, R, W, _, _),
    "dvae_kl_finish": (RW, _, R, _),
    "dvae_u8_to_f32": (R, W, _),
    "dvae_btcvae_fwd": (R, R, R, _, _, _, _, _, R, W, W),
    "dvae_btcvae_bwd": (R, R, R, R, _, _, _, _, _, R, R, R, W, W, W),
    "dvae_permute_dims": (R, R, W, _, _),
    "dvae_disc_losses": (R, _, R, W, W, W),
    "dvae_loss_pack": (R, R, _, R, _, R, W),
    "dvae_loss_finalize": (_, R, _, _, R, W),
    "dvae_loss_epilogue": (_, R, R, _, _, R, _, R, _, R, W, W),
    # the host side's element-wise glue and torch ops (parallel.scale_ / copy_flat_, _lib.record_py: fn name, self, arguments)
    "scale_": (RW, _),
    "copy_flat_": (W, R),
    # collectives (tests/step_trace.FakeComm): in place over a span, or from / into named buffers
    "all_reduce": (RW,),
    "all_reduce_async": (RW,),
    "all_reduce_cols_sums": (RW, _, _, _),
    "all_gather_latents": (R, R, R, W),
    "all_gather_rows": (R, W),
}
# entries recorded by content: their accesses are worked out by name in _accesses
SPECIAL = ("dvae_stage_weights", "dvae_fc_chain_fwd", "dvae_fc_chain_bwd", "dvae_linear_wgrad_grouped", "py",
           # what the checker adds between two steps: the host's logging read, the optimizers, the next batch
           "host_read", "optim.step", "next_batch",
           # markers of schedule_trace: the loss plugins' FC chain (accesses: the test's chain_marker), a fired fork hook
           "fc_chain", "hook")
ORDERING = ("dvae_stream_order", "dvae_event_record", "dvae_event_wait", "wait")
# the header's two `const` arguments that tests/test_step_schedule.WRITES lists as written (the header and csrc/capi.hip agree)
CONST_IN_HEADER = {("dvae_loss_epilogue", 2), ("dvae_btcvae_bwd", 11)}

# the argument structs of the FC chains by field (dvae_fc_chain_fwd_args / dvae_fc_chain_bwd_args); a field the trace leaves
# out points at the buffer of its own name (step_trace._entry)
FC_FWD = dict(a_flat=R, w_e1=R, w_e2=R, w_ml=R, w_d1=R, w_d2=R, w_d3=R, b_e1=R, b_e2=R, b_ml=R, b_d1=R, b_d2=R, b_d3=R, eps=R,
              h1=W, h2=W, ml=W, mu=W, logvar=W, z=W, kl_part=W, d1=W, d2=W, d3=W, n_enc=_, n_kl=_, n_dec=_, D=_,
              conv_in=R, conv_w=R, conv_b=R, convT_w=R, convT_b=R, convT_out=W)
FC_BWD = dict(gd3=R, w_d3=R, w_d2=R, w_d1=R, w_ml=R, w_e2=R, w_e1=R, d2=R, d1=R, h2=R, h1=R, a_flat=R, mu=R, logvar=R, eps=R,
              dz2=R, dz3=R, dmu_x=R, dlv_x=R, scal=R, coef=R, gd2=W, gd1=W, dz=W, dml=W, gh2=W, gh1=W, ga_flat=W, n=_, D=_,
              convT_gout=R, convT_w=R, d3=R, conv_w=R, conv_act=R, conv_gin=W)
# with the fused 4x4 ends a chain launch WRITES what it otherwise reads
FC_FWD_ENDS = {"conv_in": ("a_flat", W)}
FC_BWD_ENDS = {"convT_gout": ("gd3", W)}
# fields a launch always passes (engine.fc_chain_fwd / fc_chain_bwd); the fused-ends fields only when the trace shows them
FC_FWD_ALWAYS = [k for k in FC_FWD if not k.startswith("conv")]
FC_BWD_ALWAYS = [k for k in FC_BWD if not k.startswith("conv") and k != "d3"]
GROUPED = (R, R, W, W, _, _, _)           # one problem of dvae_linear_wgrad_grouped: x, dy, dw, db, M, K, N

# strings that are no pointers: row-count symbols, the event slot, a collective's "all", the torch method of a "py" entry
SCALARS = {"B", "WB", "Bh", "2Bh", "WBh", "slot", "all", "numel(x)", "normal_", "copy_", "vae", "disc"}
SCALAR_PREFIXES = ("klb(", "1/(")
STREAMS = ("main", "side", "wg2", "aux", "comm")

# rows x width where the entry's own arguments give them: entry -> [(buffer argument, row argument, width)]; width: an
# argument position, a number, or "D" / "2D" (x the latent dimension)
EXTENT_ROWS = {
    "dvae_linear_fwd": [(0, 4, 5), (3, 4, 6)],
    "dvae_linear_dgrad": [(0, 5, 7), (2, 5, 6), (4, 5, 6)],
    "dvae_linear_wgrad": [(0, 4, 5), (1, 4, 6)],
    "dvae_permute_dims": [(0, 3, 4), (2, 3, 4)],
    "dvae_reparam_kl_fwd": [(0, 7, "2D"), (1, 7, "D"), (2, 7, "D"), (3, 7, "D"), (4, 7, "D")],
    "dvae_reparam_kl_bwd": [(i, 11, "D") for i in range(8)] + [(10, 11, "2D")],
    "dvae_btcvae_fwd": [(0, 3, "D"), (1, 3, "D"), (2, 3, "D")],
    "dvae_btcvae_bwd": [(0, 4, "D"), (1, 4, "D"), (2, 4, "D"), (12, 7, "D"), (13, 4, "D"), (14, 4, "D")],
}
ARENAS = ("dg:", "dp:", "g:", "p:")
INF = float("inf")

Access = namedtuple("Access", "base lo hi mode arg")
Hazard = namedtuple("Hazard", "kind i j buf")


class Unclassified(AssertionError):
    """An entry name without a row in ACCESS, or an argument that is neither classified nor a listed scalar."""


def is_scalar(s):
    return s in SCALARS or s in STREAMS or s.startswith(SCALAR_PREFIXES)


class Context:
    """What the names of one traced case mean: arenas ({"g:": ParamArena, ...}: the offsets of the slices), sizes ({"B": rows,
    "Bh": ..., "D": latent_dim}), chain_marker ((reads, writes) of schedule_trace's "fc_chain" marker)."""

    def __init__(self, arenas=None, sizes=None, chain_marker=((), ())):
        self.arenas, self.sizes, self.chain_marker = arenas or {}, sizes or {}, chain_marker

    def rows(self, v):
        """A row-count symbol or number -> rows (None: unknown)."""
        if isinstance(v, int) and not isinstance(v, bool):
            return v
        s = self.sizes
        W_ = s.get("W", 1)
        return {"B": s.get("B"), "WB": s.get("B") and s["B"] * W_, "Bh": s.get("Bh"), "2Bh": s.get("Bh") and 2 * s["Bh"],
                "WBh": s.get("Bh") and s["Bh"] * W_}.get(v)


_PTR = re.compile(r"(.+?)\+(\d+)(?:(Bh|B)D)?$")


def locate(s, ctx, length=None):
    """A pointer name -> (base buffer, lo, hi) in elements; hi = INF where the extent is unknown.  length: elements from the
    pointer on (None: unknown -- a slice of an arena: the whole slice)."""
    off, m = 0, _PTR.match(s)
    if m:
        s, off = m.group(1), int(m.group(2))
        if m.group(3):
            off *= ctx.sizes[m.group(3)] * ctx.sizes["D"]
    for prefix in ARENAS:
        if s.startswith(prefix):
            arena = ctx.arenas.get(prefix)
            if arena is None:
                break
            lo, n = arena.offsets[s[len(prefix):]]
            if length is None and not off:
                length = n
            return prefix, lo + off, INF if length is None else lo + off + length
    if s.startswith("img:"):          # the weight images: ONE buffer (engine._Images.buf), rewritten whole by dvae_stage_weights
        return "img", 0, INF
    return s, off, INF if length is None else off + length


def _span(v, ctx):
    name, n = v
    return locate(name, ctx, None if n == "all" else n)


def _accesses(e, ctx):
    """[Access] of one launch / collective entry (its trailing stream already taken off by the caller)."""
    name, args = e[0], e[1:-1]
    out = []

    def add(s, mode, length=None):
        if s is None or mode is None:
            return
        if not isinstance(s, str) or is_scalar(s):
            raise Unclassified("%r: argument %r stands where a pointer is expected" % (e, s))
        out.append(Access(*(locate(s, ctx, length) + (mode, s))))

    def scalar(v):
        if isinstance(v, str) and not is_scalar(v):
            raise Unclassified("%r: the string %r is neither classified as a buffer nor a listed scalar" % (e, v))
        if isinstance(v, list):
            raise Unclassified("%r: the structured argument %r is not classified" % (e, v))

    if name in ACCESS:
        row = ACCESS[name]
        if len(row) != len(args):
            raise Unclassified("%r: %d arguments, ACCESS lists %d" % (e, len(args), len(row)))
        lengths = {}
        for buf, rows, width in EXTENT_ROWS.get(name, ()):
            n = ctx.rows(args[rows])
            D = ctx.sizes.get("D")
            w = (D and D * len(width)) if isinstance(width, str) else args[width]        # "D" / "2D": 1 x / 2 x latent_dim
            if n is not None and isinstance(w, int):
                lengths[buf] = n * w
        for i, (mode, v) in enumerate(zip(row, args)):
            if mode is None:
                scalar(v)
            elif isinstance(v, list):            # a collective's ["name", elements or "all"]
                out.append(Access(*(_span(v, ctx) + (mode, v[0]))))
            else:
                add(v, mode, lengths.get(i))
    elif name == "dvae_stage_weights":           # (convs, FCs, thin layer?, coef, the coefficients): every image <- the parameters
        for v in args[:3]:
            scalar(v)
        out.append(Access("img", 0, INF, W, "img:*"))
        out.append(Access("p:", 0, INF, R, "p:*"))
        add(args[3], W)
        for v in args[4] or ():
            scalar(v)
    elif name in ("dvae_fc_chain_fwd", "dvae_fc_chain_bwd"):
        fwd = name.endswith("fwd")
        table, always, ends = (FC_FWD, FC_FWD_ALWAYS, FC_FWD_ENDS) if fwd else (FC_BWD, FC_BWD_ALWAYS, FC_BWD_ENDS)
        shown = dict((k, v) for k, v in args[0][1:])
        if args[0][0] != ("FcChainFwdArgs" if fwd else "FcChainBwdArgs") or set(shown) - set(table):
            raise Unclassified("%r: fields %s are not classified" % (e, sorted(set(shown) - set(table))))
        fields = dict((k, k) for k in always)
        if not fwd and "convT_gout" in shown:
            fields["d3"] = "d3"
        fields.update(shown)
        modes = dict(table)
        for trigger, (field, mode) in ends.items():
            if shown.get(trigger) is not None:
                modes[field] = mode
        for k, v in fields.items():
            if modes[k] is None:
                scalar(v)
            else:
                add(v, modes[k])
    elif name == "dvae_linear_wgrad_grouped":
        scalar(args[1])
        for prob in args[0]:
            n = ctx.rows(prob[4])
            for i, (mode, v) in enumerate(zip(GROUPED, prob)):
                if mode is None:
                    scalar(v)
                else:
                    add(v, mode, n * prob[5 + i] if (i < 2 and n is not None) else None)
    elif name == "py":                           # (torch method, self, arguments): self <- f(arguments)
        scalar(args[0])
        add(args[1], W)
        for v in args[2:]:
            add(v, R)
    elif name == "host_read":
        add(args[0], R)
    elif name == "next_batch":
        add(args[0], W)
    elif name == "optim.step":                   # Adam over one arena: p <- f(p, g)
        prefix = {"vae": "", "disc": "d"}[args[0]]
        out.append(Access(prefix + "p:", 0, INF, RW, prefix + "p:*"))
        out.append(Access(prefix + "g:", 0, INF, R, prefix + "g:*"))
    elif name == "fc_chain":
        for s in ctx.chain_marker[0]:
            add(s, R)
        for s in ctx.chain_marker[1]:
            add(s, W)
    elif name != "hook":
        raise Unclassified("%r: the entry name has no row in the access table" % (e,))
    return out


def accesses(e, ctx):
    """(stream, [Access]) of a launch / collective entry; schedule_trace's markers run on the main stream."""
    if e[0] in ("fc_chain", "hook"):
        return "main", _accesses(list(e) + ["main"], ctx)
    return e[-1], _accesses(e, ctx)


def between_steps(trace, train, factor):
    """What the host does between two steps of one case, as entries on the main stream: the logging read of the scalars, the
    optimizer(s) (models/losses.py: fused_step / call_optimize; the discriminator's behind the VAE's) and the next batch."""
    out = [["host_read", "scal", "main"]]
    if train:
        out.append(["optim.step", "vae", "main"])
        if factor:
            out.append(["optim.step", "disc", "main"])
    if any("x" in e[1:-1] for e in trace if isinstance(e, list) and e[0] not in ORDERING):
        out.append(["next_batch", "x", "main"])
    return out


def _kind(first, second):
    if first == R:
        return "WAR"
    return "RAW" if second == R else "WAW"


def check(trace, ctx):
    """[Hazard] of a trace: every pair of entries i < j on different streams with conflicting accesses where i does not
    happen-before j (one Hazard per pair and base buffer)."""
    clock = {}           # stream -> {stream: tick}: what everything issued on it from now on is ordered behind
    marks = {}           # an event slot / an asynchronous collective's span -> the clock it carries
    hist = {}            # base buffer -> [(entry, stream, tick, lo, hi, mode)]
    hazards, seen = [], set()

    def clk(s):
        return clock.setdefault(s, {s: 0})

    def merge(into, frm):
        for s, t in frm.items():
            if into.get(s, 0) < t:
                into[s] = t

    def run(j, stream, accs):
        c = clk(stream)
        c[stream] += 1
        tick = c[stream]
        for a in accs:
            h = hist.setdefault(a.base, [])
            ordered = True
            for (i, s_i, t_i, lo, hi, mode) in h:
                if s_i == stream or (mode == R and a.mode == R) or a.hi <= lo or hi <= a.lo:
                    continue
                if c.get(s_i, 0) < t_i:
                    ordered = False
                    if (i, j, a.base) not in seen:
                        seen.add((i, j, a.base))
                        hazards.append(Hazard(_kind(mode, a.mode), i, j, a.base))
            if a.mode != R and ordered and a.lo == 0 and a.hi == INF:
                # a whole-buffer write behind everything before it: whatever conflicts with those conflicts with this, and is
                # ordered behind them if it is ordered behind this
                del h[:]
            elif a.mode == R:
                # the same read again on the same stream: the later one stands for both
                h[:] = [x for x in h if not (x[1] == stream and x[5] == R and x[3] == a.lo and x[4] == a.hi)]
            h.append((j, stream, tick, a.lo, a.hi, a.mode))

    for j, e in enumerate(trace):
        name = e[0]
        if name == "dvae_stream_order":
            merge(clk(e[2]), clk(e[1]))
        elif name == "dvae_event_record":
            marks[("slot", e[1])] = dict(clk(e[-1]))
        elif name == "dvae_event_wait":
            merge(clk(e[-1]), marks.get(("slot", e[1]), {}))
        elif name == "all_reduce_async":
            merge(clk("comm"), clk(e[-1]))
            run(j, "comm", _accesses(e, ctx))
            marks[("span", str(e[1]))] = dict(clk("comm"))
        elif name == "wait":
            merge(clk(e[-1]), marks.get(("span", str(e[1])), {}))
        else:
            run(j, *accesses(e, ctx))
    return hazards


def show(trace):
    return "\n".join("  %2d %s" % (i, e) for i, e in enumerate(trace))


def describe(label, trace, hazards):
    """The failure message: per hazard its kind, the buffer and both entries; then the trace."""
    lines = ["%s: %d unordered cross-stream hazard(s)" % (label, len(hazards))]
    for h in hazards:
        lines.append("  %s on %s: entry %d is not ordered behind entry %d\n    %2d %s\n    %2d %s"
                     % (h.kind, h.buf, h.j, h.i, h.i, trace[h.i], h.j, trace[h.j]))
    return "\n".join(lines) + "\nthe whole trace:\n" + show(trace)


# ---- the header, for the test that holds ACCESS to it --------------------------------------------------------------------------
def _header():
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dvae_hip.h")) as f:
        return re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)


def header_struct_fields(struct):
    """{field: (is pointer, is const)} of one `typedef struct { ... } struct;` of include/dvae_hip.h."""
    body = re.search(r"typedef struct \{([^}]*)\}\s*%s;" % struct, _header()).group(1)
    fields = {}
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        for name in re.sub(r"^(const\s+)?\w+\s*\**", "", decl).split(","):
            fields[name.strip().lstrip("*").strip()] = ("*" in decl, decl.startswith("const"))
    return fields


def header_prototypes():
    """{entry point: [(is pointer, is const)] per parameter, `stream` excluded} of include/dvae_hip.h."""
    text = _header()
    out = {}
    for name, params in re.findall(r"\bint\s+(dvae_\w+)\s*\(([^)]*)\)\s*;", text):
        ps = [p.strip() for p in params.split(",") if p.strip() and p.strip() != "void"]
        out[name] = [("*" in p, p.startswith("const")) for p in ps if not p.endswith(" stream")]
    return out
