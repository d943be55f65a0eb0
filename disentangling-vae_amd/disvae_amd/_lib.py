"""ctypes binding of libdvae_hip.so (the C-ABI declared in include/dvae_hip.h).

The library is the product: there is NO CPU or PyTorch fallback.  If the shared object is
missing or a symbol cannot be resolved, importing an op fails loudly.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DVAE_HIP_LIB", os.path.join(_HERE, "..", "lib", "libdvae_hip.so"))

NCHW, NHWC = 0, 1
ACT_NONE, ACT_RELU, ACT_LEAKY02, ACT_SIGMOID = 0, 1, 2, 3
REC = {"bernoulli": 0, "gaussian": 1, "laplace": 2}
LOSS_BETAH, LOSS_BETAB, LOSS_BTCVAE, LOSS_FACTOR = 0, 1, 2, 3
# scalar slots (dvae_hip.h)
S_LOSS, S_REC, S_KL, S_KL0, S_MI, S_TC, S_DWKL, S_KLW, S_DTC, NSCAL = 0, 1, 2, 3, 19, 20, 21, 22, 23, 32
C_INV_B, C_ANNEAL, C_BETA, C_ALPHA, C_GAMMA, C_CAP, NCOEF = 0, 1, 2, 3, 4, 5, 8
REC_NPART = 2048
NPACK = 32
MAX_LATENT_DIM = 16          # DVAE_MAX_D: the FUSED kernels (FC chain, register-resident estimator, 16-wide KL records)
ROWSTATS = 32                # DVAE_ROWSTATS
WIDE_KL0 = 32                # DVAE_WIDE_KL0


# Layouts that depend on the latent dimension (include/dvae_hip.h: above DVAE_MAX_D the same entry points run the run-time-D
# kernels of csrc/latent_wide.hip on "wide" buffers)
def wide(D):
    return D > MAX_LATENT_DIM


def rowstats_stride(D):
    """DVAE_ROWSTATS_STRIDE(D)."""
    return ROWSTATS if D <= MAX_LATENT_DIM else (D + 4 + 3) & ~3


def btcvae_tmp_floats(Bg, Bl, D):
    """DVAE_BTCVAE_TMP_FLOATS(Bg, Bl, D)."""
    return 3 * D * Bg + (0 if D <= MAX_LATENT_DIM else Bl * Bg)


def npack(D):
    """DVAE_NPACK_D(D)."""
    return NPACK if D <= MAX_LATENT_DIM else NPACK + D


def nscal(D):
    """DVAE_NSCAL_D(D)."""
    return NSCAL if D <= MAX_LATENT_DIM else NSCAL + D


def kl0(D):
    """First per-dimension KL slot of scal[] (DVAE_S_KL0, or DVAE_WIDE_KL0 above DVAE_MAX_D)."""
    return S_KL0 if D <= MAX_LATENT_DIM else WIDE_KL0

_p = ctypes.c_void_p
_i = ctypes.c_int
_l = ctypes.c_long

# name -> argtypes (all return int unless listed in _RESTYPE)
SIGNATURES = {
    "dvae_version": [],
    "dvae_last_error": [],
    "dvae_conv4s2_fwd": [_p, _i, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _p],
    "dvae_conv4s2_dgrad": [_p, _i, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p],
    "dvae_conv4s2_wgrad": [_p, _i, _p, _i, _p, _p, _i, _i, _i, _i, _i, _p, _p],
    "dvae_convT4s2_fwd": [_p, _i, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _p],
    "dvae_convT4s2_dgrad": [_p, _i, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p],
    "dvae_convT4s2_wgrad": [_p, _i, _p, _i, _p, _p, _i, _i, _i, _i, _i, _p, _p],
    "dvae_convT4s2_sigmoid_recon_fwd": [_p, _i, _p, _p, _p, _p, _p, _i, _p, _p, _i, _i, _i, _i, _i, _p],
    "dvae_conv_wgrad_ws_floats": [],
    "dvae_stage_weights": [_p, _i, _p, _i, _p, _p, _p, _p],
    "dvae_convT3_fwd_staged": [_p, _p, _p, _p, _i, _p, _p, _i, _p, _p, _i, _i, _p],
    "dvae_conv32_down": [_p, _p, _p, _p, _p, _i, _i, _i, _i, _p],
    "dvae_conv32_up": [_p, _i, _p, _p, _p, _p, _i, _i, _i, _p],
    "dvae_conv1_fwd_bits": [_p, _i, _p, _p, _p, _p, _i, _i, _p],
    "dvae_conv32_up_bits": [_p, _p, _p, _p, _p, _p, _i, _i, _p],
    "dvae_convT3_dgrad_bits": [_p, _p, _p, _p, _i, _i, _p],
    "dvae_fc_chain_fwd": [_p, _p],
    "dvae_fc_chain_bwd": [_p, _p],
    "dvae_fc_chain_rows": [_i],
    "dvae_reparam_kl_blocks": [_i],
    "dvae_kl_finish": [_p, _i, _p, _i, _p],
    "dvae_u8_to_f32": [_p, _p, _l, _p],
    "dvae_u8_fused_supported": [_i, _i, _i],
    "dvae_conv4s2_fwd_u8": [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p],
    "dvae_conv4s2_wgrad_u8": [_p, _p, _p, _p, _i, _i, _i, _i, _i, _p, _p],
    "dvae_convT4s2_sigmoid_recon_fwd_u8": [_p, _p, _p, _p, _p, _p, _i, _p, _p, _i, _i, _i, _i, _i, _p],
    "dvae_relayout": [_p, _i, _p, _i, _i, _i, _i, _p],
    "dvae_linear_fwd": [_p, _p, _p, _p, _i, _i, _i, _i, _p, _p],
    "dvae_linear_dgrad": [_p, _p, _p, _i, _p, _i, _i, _i, _p, _p],
    "dvae_linear_wgrad": [_p, _p, _p, _p, _i, _i, _i, _p, _p],
    "dvae_linear_wgrad_grouped": [_p, _i, _p],
    "dvae_reparam_kl_fwd": [_p, _p, _p, _p, _p, _p, _p, _i, _i, _p],
    "dvae_reparam_kl_bwd": [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _p],
    "dvae_recon_loss": [_p, _p, _l, _i, _p, _p, _p, _i, _p],
    "dvae_kl_normal_bwd": [_p, _p, _p, _p, _p, _i, _i, _p],
    "dvae_reduce_sum": [_p, _l, ctypes.c_float, _p, _p],
    "dvae_sigmoid_bwd": [_p, _p, _p, _l, _p],
    "dvae_btcvae_fwd": [_p, _p, _p, _i, _i, _i, _i, _i, _p, _p, _p, _p],
    "dvae_btcvae_bwd": [_p, _p, _p, _p, _i, _i, _i, _i, _i, _p, _p, _p, _p, _p, _p, _p],
    "dvae_permute_dims": [_p, _p, _p, _i, _i, _p],
    "dvae_latent_entropy_ws_floats": [_l, _i, _i],
    "dvae_latent_entropy": [_p, _p, _p, _l, _i, _i, _p, _p, _p],
    "dvae_disc_losses": [_p, _i, _p, _p, _p, _p, _p],
    "dvae_loss_pack": [_p, _p, _i, _p, _i, _p, _p, _p],
    "dvae_loss_finalize": [_i, _p, _i, _i, _p, _p, _p],
    "dvae_loss_epilogue": [_i, _p, _p, _i, _i, _p, _i, _p, _i, _p, _p, _p, _p],
    "dvae_set_coef": [_p] + [ctypes.c_float] * 8 + [_p],
    "dvae_comm_load": [ctypes.c_char_p],
    "dvae_comm_unique_id": [_p],
    "dvae_comm_init": [_p, _p, _i, _i],
    "dvae_comm_destroy": [_p],
    "dvae_comm_world": [_p],
    "dvae_comm_rank": [_p],
    "dvae_comm_allreduce": [_p, _p, _l, _p],
    "dvae_comm_allgather": [_p, _p, _p, _l, _p],
    "dvae_comm_reducescatter": [_p, _p, _p, _l, _p],
    "dvae_comm_broadcast": [_p, _p, _l, _i, _p],
    "dvae_comm_group_start": [],
    "dvae_comm_group_end": [],
    "dvae_add": [_p, _p, _p, _l, _p],
    "dvae_adam_step": [_p, _i, ctypes.c_float, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                       ctypes.c_double, _p],
    "dvae_axpby": [_p, _p, ctypes.c_float, _p, ctypes.c_float, _l, _p],
    "dvae_swap_outer": [_p, _p, _i, _i, _l, _p],
    "dvae_image_grid_u8": [_p, _l, _i, _i, _i, _i, _i, ctypes.c_float, _i, _p, _p],
    "dvae_image_grid_shape": [_l, _i, _i, _i, _i, _i, _p, _p],
    "dvae_recon_rows_ws_floats": [_l, _i, _l, _p],
    "dvae_recon_rows": [_p, _p, _i, _l, _i, _l, _i, _p, _p, _p],
    "dvae_iw_loglik": [_p, _p, _p, _p, _p, _l, _i, _i, _i, _i, _i, _p, _p, _p, _p],
    "dvae_stream_order": [_p, _p],
    "dvae_stream_create": [_p],
    "dvae_event_record": [_i, _p],
    "dvae_event_wait": [_i, _p],
    "dvae_plan_op": [ctypes.c_char_p],
    "dvae_plan_run": [_p, _i],
}
_RESTYPE = {"dvae_last_error": ctypes.c_char_p, "dvae_conv_wgrad_ws_floats": ctypes.c_size_t,
            "dvae_latent_entropy_ws_floats": ctypes.c_size_t}


FCW_MAX = 8
KL_MAX_BLOCKS = 8192                 # DVAE_KL_MAX_BLOCKS
KL_FLOATS = 16 + KL_MAX_BLOCKS * 16   # DVAE_KL_FLOATS
FC_CHAIN_MAX_ROWS = 8 * KL_MAX_BLOCKS  # rows one dvae_fc_chain_* launch takes


def fc_chain_rows(n):
    """dvae_fc_chain_rows(n): batch rows per workgroup of dvae_fc_chain_* over n rows = granularity of its KL partial blocks."""
    return int(lib().dvae_fc_chain_rows(int(n)))



class ConvImageDesc(ctypes.Structure):
    """dvae_conv_image_desc (include/dvae_hip.h)."""
    _fields_ = [("w", _p), ("img_down", _p), ("img_up", _p)]


class FcImageDesc(ctypes.Structure):
    """dvae_fc_image_desc (include/dvae_hip.h)."""
    _fields_ = [("w", _p), ("img_fwd", _p), ("img_bwd", _p), ("N", _i), ("K", _i)]


class ThinImageDesc(ctypes.Structure):
    """dvae_thin_image_desc (include/dvae_hip.h)."""
    _fields_ = [("w", _p), ("img_pairs", _p), ("C", _i)]


def thin_pair_floats(C):
    """DVAE_THIN_PAIR_FLOATS(C)."""
    return 112 if C == 3 else 16


class FcChainFwdArgs(ctypes.Structure):
    """dvae_fc_chain_fwd_args (include/dvae_hip.h)."""
    _fields_ = [(n_, _p) for n_ in ("a_flat", "w_e1", "w_e2", "w_ml", "w_d1", "w_d2", "w_d3", "b_e1", "b_e2", "b_ml",
                                    "b_d1", "b_d2", "b_d3", "eps", "h1", "h2", "ml", "mu", "logvar", "z", "kl_part",
                                    "d1", "d2", "d3")] + [(n_, _i) for n_ in ("n_enc", "n_kl", "n_dec", "D")] + \
               [(n_, _p) for n_ in ("conv_in", "conv_w", "conv_b", "convT_w", "convT_b", "convT_out")]


class FcChainBwdArgs(ctypes.Structure):
    """dvae_fc_chain_bwd_args (include/dvae_hip.h)."""
    _fields_ = [(n_, _p) for n_ in ("gd3", "w_d3", "w_d2", "w_d1", "w_ml", "w_e2", "w_e1", "d2", "d1", "h2", "h1",
                                    "a_flat", "mu", "logvar", "eps", "dz2", "dz3", "dmu_x", "dlv_x", "scal", "coef",
                                    "gd2", "gd1", "dz", "dml", "gh2", "gh1", "ga_flat")] + [("n", _i), ("D", _i)] + \
               [(n_, _p) for n_ in ("convT_gout", "convT_w", "d3", "conv_w", "conv_act", "conv_gin")]


def struct_of(cls, **kw):
    """ctypes struct with the given fields (device pointers as ints / None, sizes as ints) -> (struct, its address).
    Keep the struct alive while a recorded launch plan may replay the call."""
    st = cls()
    for k, v in kw.items():
        setattr(st, k, v)
    return st, ctypes.addressof(st)


class AdamTensor(ctypes.Structure):
    """dvae_adam_tensor (include/dvae_hip.h)."""
    _fields_ = [("p", _p), ("g", _p), ("m", _p), ("v", _p), ("step", _p), ("n", _l)]


class LinearWgradDesc(ctypes.Structure):
    """dvae_linear_wgrad_desc (include/dvae_hip.h)."""
    _fields_ = [("x", _p), ("dy", _p), ("dw", _p), ("db", _p), ("M", _i), ("K", _i), ("N", _i)]


def wgrad_descs(problems):
    """[(x, dy, dw, db, M, K, N), ...] (device pointers as ints) -> (host array, its address).  The array must stay
    alive as long as a recorded launch plan may replay the call: callers keep it."""
    arr = (LinearWgradDesc * len(problems))()
    for d, (x, dy, dw, db, M, K, N) in zip(arr, problems):
        d.x, d.dy, d.dw, d.db, d.M, d.K, d.N = x, dy, dw, db, M, K, N
    return arr, ctypes.addressof(arr)


class DvaeHipError(RuntimeError):
    pass


_lib = None


def lib():
    """Load (once) and return the ctypes handle; raises if the HIP library is absent."""
    global _lib
    if _lib is None:
        path = os.path.abspath(LIB_PATH)
        if not os.path.exists(path):
            raise DvaeHipError(
                "libdvae_hip.so not found at %s -- build it with `python disentangling-vae_amd/build.py` "
                "(there is no CPU / PyTorch fallback for the training-step kernels)" % path)
        h = ctypes.CDLL(path)
        for name, argtypes in SIGNATURES.items():
            fn = getattr(h, name)  # AttributeError if the symbol is missing: fail loudly
            fn.argtypes = argtypes
            fn.restype = _RESTYPE.get(name, ctypes.c_int)
        _lib = h
    return _lib


EVENT_SLOTS = 16              # DVAE_EVENT_SLOTS
_next_slot = [0]


def next_event_slot():
    """dvae_event_record / dvae_event_wait slot for one loss object: handed out round-robin so that two trainers on one
    device (different streams, different host threads) do not wait on each other's marks."""
    s = _next_slot[0] % EVENT_SLOTS
    _next_slot[0] += 1
    return s


def new_stream(device):
    """A torch handle (ExternalStream) of a stream made by dvae_stream_create on `device`: see include/dvae_hip.h for why the
    engine's streams do not come from torch's pool."""
    import torch
    with torch.cuda.device(device):
        h = ctypes.c_void_p()
        call("dvae_stream_create", ctypes.addressof(h))
        return torch.cuda.ExternalStream(h.value, device=device)


ALLOC_GEN = [0]   # bumped whenever the engine (re)allocates device buffers: recorded plans hold raw pointers


def note_alloc():
    ALLOC_GEN[0] += 1


PLAN_MAX_ARGS = 20                   # DVAE_PLAN_MAX_ARGS


class PlanEntry(ctypes.Structure):
    """dvae_plan_entry (include/dvae_hip.h)."""
    _fields_ = [("op", _i), ("nargs", _i), ("args", ctypes.c_uint64 * PLAN_MAX_ARGS)]


_REC = None      # launch list being recorded (graph.py: "plan" replay), or None
_OPS = {}        # entry point name -> dvae_plan_op code (-1: not replayable from C)


def _pack(ctype, v):
    """One argument of a recorded call as the 64 bits dvae_plan_run unpacks (pointers / integers by value, floats as their
    fp32 bit pattern)."""
    if v is None:
        return 0
    if ctype is ctypes.c_float:
        return ctypes.c_uint32.from_buffer_copy(ctypes.c_float(v)).value
    if ctype not in (_p, _i, _l):
        # dvae_plan_run decodes pointers / integers by value and every floating-point parameter from an fp32 bit pattern: a
        # double (or any other type) would replay silently truncated
        raise DvaeHipError("arguments of type %s cannot be recorded in a launch plan" % getattr(ctype, "__name__", ctype))
    if isinstance(v, (bytes, float)):
        raise DvaeHipError("%s argument for a %s parameter cannot be recorded" % (type(v).__name__, ctype.__name__))
    return int(v) & 0xFFFFFFFFFFFFFFFF


TRACE = None     # measurement hook (bench.py): {"names": set of entry points, "out": list} -> every matching launch is bracketed
                 # by HIP events on ITS stream (the last argument) and appended as (name, args, start_event, end_event)


def call(name, *args):
    """Call an int-returning entry point, raise on a non-zero status."""
    h = lib()
    fn = getattr(h, name)
    if TRACE is not None and name in TRACE["names"] and _REC is None:
        import torch
        st = torch.cuda.ExternalStream(args[-1]) if args[-1] else torch.cuda.current_stream()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        rc = fn(*args)
        e1.record(st)
        TRACE["out"].append((name, args, e0, e1))
        if rc != 0:
            raise DvaeHipError("%s failed (%d): %s" % (name, rc, h.dvae_last_error().decode()))
        return
    if _REC is not None:
        # frozen copy of the launch: the arguments as 64-bit words (replayed by dvae_plan_run, one foreign call per run of
        # consecutive entry-point calls) when the entry point is replayable, else pre-converted to their ctypes
        op = _OPS.get(name)
        if op is None:
            op = _OPS[name] = h.dvae_plan_op(name.encode())
        if len(args) != len(fn.argtypes):
            raise DvaeHipError("%s takes %d arguments, got %d" % (name, len(fn.argtypes), len(args)))
        if op >= 0 and len(args) <= PLAN_MAX_ARGS:
            _REC.append(("c", op, tuple(_pack(t, a) for t, a in zip(fn.argtypes, args)), name))
        else:
            _REC.append(("f", fn, tuple(None if a is None else t(a) for t, a in zip(fn.argtypes, args)), name))
    rc = fn(*args)
    if rc != 0:
        raise DvaeHipError("%s failed (%d): %s" % (name, rc, h.dvae_last_error().decode()))


def record_py(fn, *args):
    """Run a host-side callable that belongs to the launch sequence (stream fork/join, a torch
    copy) and keep it in the recorded plan."""
    if _REC is not None:
        _REC.append(("p", fn, args, None))
    return fn(*args)


def record_on_stream(fn, *args):
    """record_py for a torch op (or a torch.distributed collective) that goes to torch's CURRENT stream: the loss plugins
    issue part of an iteration under ``with torch.cuda.stream(side)``, so a replay re-enters the stream that was current when
    the op was recorded."""
    if _REC is not None:
        import torch
        st = torch.cuda.current_stream()

        def run():
            with torch.cuda.stream(st):
                fn(*args)
        _REC.append(("p", run, (), None))
    return fn(*args)


def begin_record():
    global _REC
    _REC = []


def end_record():
    """-> the plan: a list of segments, ("c", PlanEntry array, n, names) for a run of replayable entry-point calls,
    ("f", fn, args, name) for a foreign call that is not, ("p", fn, args) for a host-side callable."""
    global _REC
    rec, _REC = _REC, None
    plan, run = [], []

    def flush():
        if run:
            arr = (PlanEntry * len(run))()
            for e, (_, op, words, _) in zip(arr, run):
                e.op, e.nargs = op, len(words)
                for i, w in enumerate(words):
                    e.args[i] = w
            plan.append(("c", arr, len(run), tuple(r[3] for r in run)))
            del run[:]

    for ent in rec:
        if ent[0] == "c":
            run.append(ent)
        else:
            flush()
            plan.append(ent)
    flush()
    return plan


def replay(plan):
    h = lib()
    for seg in plan:
        kind = seg[0]
        if kind == "c":
            rc = h.dvae_plan_run(ctypes.addressof(seg[1]), seg[2])
            if rc != 0:
                raise DvaeHipError("replay of %d recorded launches failed (%d): %s" % (seg[2], rc, h.dvae_last_error().decode()))
        elif kind == "f":
            rc = seg[1](*seg[2])
            if rc != 0:
                raise DvaeHipError("%s failed (%d): %s" % (seg[3], rc, h.dvae_last_error().decode()))
        else:
            seg[1](*seg[2])


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()
