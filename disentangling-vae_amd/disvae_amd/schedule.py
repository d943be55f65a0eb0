"""The launch schedule of one step as ONE immutable value.

Every decision that changes what a step issues, or on which stream, is a field (or, where it depends on the row count of one call
of the step -- FactorVAE encodes 2B rows and decodes B -- a method) of ``StepPolicy``.  ``build_policy`` is the only place that
derives them, from the step's shape and the debug switches; the thresholds below are the only ones.  The loss plugins hand the
policy to the engine once per step (``VAEEngine.begin_step``) and put the object itself into the key of a recorded plan
(``BaseLoss._replay_key``): a decision added here is in the key by construction.
"""
import functools
from typing import NamedTuple, Optional, Tuple

from . import _lib
from ._debug import knob, enabled

# how the device side of the native training iteration is issued (graph.py): None = eager Python; "plan" = recorded launch list
# (the same launches on the same streams, bit-identical results); "graph" = hipGraph; "auto" (default) = plan while the
# iteration is launch-bound (batch tensor <= AUTO_PLAN_ELEMS elements: measured cross-over), eager above.
# Sharded steps replay too: collectives are recorded plan entries (parallel.py)
# (round 6: up to 1024 images -- the same step time at 512 / 1024 images single process, 0.23-0.27 instead of 0.36 ms of host
# time per step; one rank of two of configs[3] (512 images through the sharded path) spends 0.55 ms of host per 0.63 ms step
# when it is issued eagerly: profiles/r06_s2_shard_world.txt)
AUTO_PLAN_ELEMS = 1024 * 3 * 64 * 64
# one HIP stream instead of two below this many input elements per step (StepPolicy.single_stream); DVAE_STREAMS=1|2 forces
# (round 2 measured the cross-over at 64 images, profiles/r02_run10_streams.txt; with the round-5 schedule two streams win at
# 32 and 64 images as well: 0.291 / 0.301 against 0.338 / 0.346 ms, profiles/r05_v26_sweep.txt; round 6: at 4 / 8 / 16 images
# too -- 0.306 -> 0.267, 0.312 -> 0.271, 0.315 -> 0.277 ms -- and at the 32x32 geometry level at 16 / 64 images, -3 % at 128:
# profiles/r06_s2_streams_small.txt.  Two streams at every size.)
# Small batches on one stream: below ~256 images the iteration is bound by the latency of dependent launches, a fork / join
# between hardware queues costs ~6 us each (5 forks + 1 join per iteration) and the weight-gradient kernels that the side
# stream would overlap are a few microseconds long.
SINGLE_STREAM_ELEMS = 0
# dependency-driven weight-gradient schedule (StepPolicy.eager_wgrad: a fork per layer) up to this many input elements per
# step; above, the batch-sized schedule (two forks per half of the backward pass).  Round 3 measured the two within noise
# of each other up to 384 images; with the round-5 kernels the batch-sized schedule wins at every batch measured (128
# images: 0.349 vs 0.359 ms, btcvae_dsprites 0.421 vs 0.433 ms: profiles/r05_v25_schedule_ab.txt) -- each fork costs the
# critical path an event and the small weight gradients it frees early are not what the iteration waits for.
#   batch-sized: the big layers' weight gradients are forked behind the big input gradients (two chip-filling persistent
#          kernels do not co-run: what matters is that the small kernels of the critical path find idle CUs), the tail is
#          balanced between the streams (measured at B = 1024: DESIGN.md section 5);
#   eager: every weight gradient is launched on the side stream as soon as its two operands exist (a fork per layer), beside
#          the input gradient of the same layer.  Below a few hundred images per step no kernel fills the chip, the iteration
#          is a latency chain, and the side stream should start as early as the data allows
#          (profiles/r03_v2_timeline_b128.md: backward pass 287 us against ~150 us of dependent work).
EAGER_WGRAD_ELEMS = 0
# weight gradients on TWO side streams (StepPolicy.three_streams), each launched at the first fork behind the kernel that
# produces its last operand, from this many batch rows per step (single process).  Measured
# (profiles/r06_s2_three1.txt, same box, three alternations): SLOWER for every beta-TCVAE step -- 64 / 128 / 256 / 512 / 1024
# images 0.288 -> 0.300, 0.328 -> 0.347, 0.435 -> 0.441, 0.634 -> 0.648, 1.050 -> 1.060 ms: whatever runs beside the main
# stream's chain of small kernels slows that chain by more than the side streams gain -- and faster only where the side
# stream also carries the discriminator's chain: FactorVAE from 2048 rows per step (factor 64x64x3 tensor 2048
# 1.853 -> 1.832 ms, tensor 256 0.561 -> 0.592)
THREE_STREAM_MIN_ROWS = 1 << 30
THREE_STREAM_MIN_ROWS_FACTOR = 2048
# sharded batches up to this many input elements per rank: ONE all-reduce of the whole gradient arena at the end instead of
# two overlapped spans (the step is a latency chain; every collective costs the host and both streams more than the
# overlap of 1 MB buys).  Round 6: at EVERY size -- as one rank of two (512 images) the two-span path takes 1.06-1.16 ms
# against 0.63 with one all-reduce (single process: 0.63), FactorVAE tensor 1024 / 512 per rank 1.31 / 0.93 against 1.18 / 0.83
# (profiles/r06_s2_shard_world.txt: mirrored world, C-ABI transport); the 2 MB arena is ~20 us of xGMI time, there is
# nothing worth overlapping.  (The spans stay reachable for A/B: DVAE_DEBUG=1 DVAE_SMALL_SHARD_ELEMS=<elements>.)
SMALL_SHARD_ELEMS = 1 << 40
# which encoder conv weight gradients the MAIN stream computes itself at the very end of the backward pass (after conv1's),
# instead of leaving them in the side stream's queue: the side stream is the tail of the iteration (timeline:
# profiles/r02_final_timeline.md), the main stream is idle from the end of conv1's weight gradient to the join
# (measured -1.5 %: profiles/r02_run12_tail_ab.txt).  Moving this tail to the side stream loses 2-8 % at every small batch
# (profiles/r06_s2_sched3.txt)
TAIL_MAIN = ("conv3", "conv_64")
# fused FC chain: the 8x8 <-> 4x4 layers (conv_64 / convT_64 at 64x64, conv3 / convT1 at 32x32) and their input
# gradients run INSIDE the chain launches (dvae_fc_chain_fwd / _bwd, conv_in / convT_gout fields: csrc/conv4_end.h) --
# four launches fewer on the critical path
# Up to FUSE_ENDS_MAX_ROWS rows per launch, where the step is a chain of dependent launches and each one saved counts
# (same box, three alternations, profiles/r06_s2_chain3.txt: factor 64x64x1 tensor 256 0.590 -> 0.569 ms, btcvae 64x64x3 at
# 64 / 128 / 256 images 0.311 -> 0.302, 0.347 -> 0.344, 0.450 -> 0.447 ms); from 512 rows up the fused launches -- 150 KB
# of LDS, a whole CU per workgroup -- can no longer slip in beside the other stream's persistent kernels the way the
# small conv launches do: 0.643 -> 0.652 ms at 512 images, 1.060 -> 1.082 ms at 1024 (profiles/r06_s2_chain2.txt) -- in
# the BACKWARD pass, that is; the forward chain has its own limit below
FUSE_ENDS_MAX_ROWS = 256
# the FORWARD chain's own limit: beside it the other stream carries only the estimator's small kernels, nothing a 150 KB
# workgroup could block -- 384 / 512 / 1024 images 0.545 -> 0.543, 0.631 -> 0.629, 1.039 -> 1.030 ms; level at 2048 rows,
# where the 8-row variant runs (profiles/r06_s2_fwd_ends.txt)
FUSE_ENDS_MAX_ROWS_FWD = 1024
# Round 6: convT3's weight gradient (bandwidth-bound) is forked one kernel earlier -- behind convT3's input gradient, beside
# the matrix-bound input gradient of convT2 -- instead of behind both (mode 1).  The side stream's serial chain of weight
# gradients is what small steps end on, and it now starts ~15 us sooner: 128 / 256 images 0.341 -> 0.330, 0.443 -> 0.431 ms,
# btcvae 64x64x1 B = 256 0.412 -> 0.398, 1024 images 1.054 -> 1.048 ms (profiles/r06_s2_sched2.txt).  Mode 2 (in FRONT of
# convT3's input gradient, beside it) wins another 1-2 % at 128 images and loses 1.6 % at 256, 0.7 % at 1024 (r06_s2_sched3.txt):
# used in the band below only -- the 128 images of one rank of the 8-GPU headline configuration: 0.332 -> 0.325 ms there, level
# at 32 / 64, +1.3 % at 96, +1.6 % at 256 images (profiles/r06_s2_sched3.txt, r06_s2_sched4.txt).  Not under data parallelism:
# the fork carries the late epilogue with its collectives, whose host-side issue would then stand in front of convT3's input
# gradient
EARLY_THIN_2_ROWS = (112, 128)
# steps of 129-320 images end on the side stream (its weight-gradient grid is the smaller one there, conv_wgrad_ws.hip): the
# grouped FC weight gradients become the LAST launch of the main stream's tail instead -- 256 images 0.425 -> 0.415 ms,
# btcvae 64x64x1 B = 256 0.386 -> 0.375; outside that band the main stream is the tail already: 64 / 128 / 512 / 1024
# images +1.3 / +1.4 / +2.1 / +0.6 % (profiles/r06_s2_fcw_main.txt)
FCW_MAIN_ROWS = (129, 320)

# every debug switch that shapes a step (A/B knobs: read only under DVAE_DEBUG=1, tools/README.md) with its shipped value
SWITCHES = (("DVAE_STREAMS", "auto"), ("DVAE_SINGLE_STREAM_ELEMS", str(SINGLE_STREAM_ELEMS)),
             ("DVAE_EAGER_WGRAD_ELEMS", str(EAGER_WGRAD_ELEMS)), ("DVAE_THREE_STREAM_MIN_ROWS", ""),
             ("DVAE_SMALL_SHARD_ELEMS", str(SMALL_SHARD_ELEMS)), ("DVAE_TAIL_MAIN", "default"), ("DVAE_FUSE_ENDS", "1"),
             ("DVAE_FUSE_ENDS_MAX_ROWS", str(FUSE_ENDS_MAX_ROWS)), ("DVAE_FUSE_ENDS_MAX_ROWS_FWD", str(FUSE_ENDS_MAX_ROWS_FWD)),
             ("DVAE_EARLY_THIN", "auto"), ("DVAE_FCW_MAIN", "1"), ("DVAE_FCW_MAIN_ROWS", "%d,%d" % FCW_MAIN_ROWS),
             ("DVAE_LATE_JOIN", "1"), ("DVAE_FORK_HOOK", "1"), ("DVAE_DISC_WGRAD_SIDE", "1"), ("DVAE_DISC_CHAIN2_AUX", "0"))
_SHIPPED = None


def switches():
    """The values of SWITCHES, in its order, as build_policy takes them.  Without DVAE_DEBUG=1 they are the shipped ones, read
    once (through knob(): a variable that is set but ignored is reported once)."""
    global _SHIPPED
    if enabled():
        return tuple(knob(name, default) for name, default in SWITCHES)
    if _SHIPPED is None:
        _SHIPPED = tuple(knob(name, default) for name, default in SWITCHES)
    return _SHIPPED


class StepPolicy(NamedTuple):
    single_stream: bool        # everything on the caller's stream: forks and joins do nothing
    eager_wgrad: bool          # weight gradients: dependency-driven schedule instead of the batch-sized one
    three_streams: bool        # weight gradients on two side streams (three-queue schedule)
    sharded: bool              # the step runs under data parallelism
    tail_main: Tuple[str, ...]   # encoder conv weight gradients that end the main stream
    fuse_ends: bool            # the 4x4 conv ends ride inside the FC-chain launches ...
    fuse_ends_max_rows: int    # ... of the backward chain up to this many rows
    fuse_ends_max_rows_fwd: int  # ... of the forward chain up to this many
    early_thin_wgrad: int      # where convT3's weight gradient is forked: 0 behind convT2's input gradient, 1 behind its own, 2 beside it
    early_thin_auto: bool      # mode 2 within early_thin_rows (single process), else early_thin_wgrad
    early_thin_rows: Tuple[int, int]
    fcw_main: bool             # the grouped FC weight gradients close the main stream's tail within fcw_main_rows
    fcw_main_rows: Tuple[int, int]
    grad_spans: bool           # sharded: the gradient arena is all-reduced in two overlapped spans instead of once
    late_join: bool            # the scalar epilogue runs behind the backward pass's first fork (BaseLoss._defer_loss)
    fork_hook: bool            # at_next_fork defers to the next fork (off: a fork of its own)
    disc_wgrad_side: bool      # FactorVAE: the discriminator's weight gradients on the side stream
    disc_chain2_aux: bool      # FactorVAE: the discriminator's second input-gradient chain on the exchange stream
    replay: Optional[str]      # None (eager) / "plan" / "graph"

    def ends_fwd(self, rows):
        """Does the forward chain launch over `rows` rows carry the 4x4 conv ends?"""
        return self.fuse_ends and rows <= self.fuse_ends_max_rows_fwd

    def ends(self, rows):
        """Does the backward chain launch over `rows` rows carry them?"""
        return self.fuse_ends and rows <= self.fuse_ends_max_rows

    def early_thin(self, rows):
        """Fork mode of convT3's weight gradient in a backward pass over `rows` rows."""
        if self.single_stream:
            return 0
        lo, hi = self.early_thin_rows
        return 2 if (self.early_thin_auto and lo <= rows <= hi and not self.sharded) else self.early_thin_wgrad

    def fcw_main_at(self, rows):
        return self.fcw_main and not self.single_stream and self.fcw_main_rows[0] <= rows <= self.fcw_main_rows[1]

    def three(self, chain):
        """Three-queue schedule for this backward pass (chain: the native step, fc_chain_bwd in the middle)?"""
        return bool(self.three_streams and chain and not self.single_stream and not self.eager_wgrad)


def replay_mode(setting, training, elems):
    """`setting` (a loss object's .replay: None / "plan" / "graph" / "auto") resolved for one step."""
    if not training:
        return None
    if setting == "auto":
        return "plan" if elems <= AUTO_PLAN_ELEMS else None
    return setting


@functools.lru_cache(maxsize=256)
def build_policy(img_size, latent_dim, rows, sw, world=1, kind=None, training=True, replay=None):
    """The policy of a step over `rows` images of `img_size` (a tuple) per process, `world` processes; sw: switches(), kind: the
    loss (_lib.LOSS_*; None: the autograd-compatible entry points), replay: the loss object's setting.  No decision depends on
    the input dtype.  Pure, and cached per distinct input: a step does not pay for rebuilding it."""
    sw = dict(zip((name for name, _ in SWITCHES), sw))
    elems = rows * img_size[0] * img_size[1] * img_size[2]
    factor = kind == _lib.LOSS_FACTOR
    one = sw["DVAE_STREAMS"] == "1" or (sw["DVAE_STREAMS"] == "auto" and elems <= int(sw["DVAE_SINGLE_STREAM_ELEMS"]))
    single = one and world == 1
    three_rows = sw["DVAE_THREE_STREAM_MIN_ROWS"] or (THREE_STREAM_MIN_ROWS_FACTOR if factor else THREE_STREAM_MIN_ROWS)
    tail = sw["DVAE_TAIL_MAIN"]
    return StepPolicy(
        single_stream=single,
        eager_wgrad=elems <= int(sw["DVAE_EAGER_WGRAD_ELEMS"]),
        three_streams=not one and world == 1 and rows >= int(three_rows),
        sharded=world > 1,
        tail_main=TAIL_MAIN if tail == "default" else tuple(v for v in tail.split(",") if v),
        # never above 16 latents, where the FC layers run one launch each: there is no chain launch
        fuse_ends=not _lib.wide(latent_dim) and sw["DVAE_FUSE_ENDS"] != "0",
        fuse_ends_max_rows=int(sw["DVAE_FUSE_ENDS_MAX_ROWS"]),
        fuse_ends_max_rows_fwd=int(sw["DVAE_FUSE_ENDS_MAX_ROWS_FWD"]),
        early_thin_wgrad=1 if sw["DVAE_EARLY_THIN"] == "auto" else int(sw["DVAE_EARLY_THIN"]),
        early_thin_auto=sw["DVAE_EARLY_THIN"] == "auto",
        early_thin_rows=EARLY_THIN_2_ROWS,
        fcw_main=sw["DVAE_FCW_MAIN"] == "1",
        fcw_main_rows=tuple(int(v) for v in sw["DVAE_FCW_MAIN_ROWS"].split(",")),
        grad_spans=world > 1 and elems > int(sw["DVAE_SMALL_SHARD_ELEMS"]),
        # deferred for the batch-coupled losses (behind the estimator's / the discriminator's backward kernels) and for every
        # sharded step (the all-reduce of the packed loss sums sits between its halves)
        late_join=(training and not single and (factor or kind == _lib.LOSS_BTCVAE or world > 1)
                   and sw["DVAE_LATE_JOIN"] != "0"),
        fork_hook=sw["DVAE_FORK_HOOK"] != "0",
        disc_wgrad_side=not single and sw["DVAE_DISC_WGRAD_SIDE"] != "0",
        disc_chain2_aux=not single and world == 1 and sw["DVAE_DISC_CHAIN2_AUX"] == "1",
        replay=replay_mode(replay, training, elems))
