"""Loss plugins with the API of disvae/models/losses.py (get_loss_f, BaseLoss, BetaHLoss,
BetaBLoss, FactorKLoss, BtcvaeLoss, LOSSES, RECON_DIST) on the HIP kernels, plus DipVaeLoss / DIP_LOSSES
(DIP-VAE-I / II), InfoVaeLoss / INFO_LOSSES (InfoVAE / MMD-VAE) and WeakVaeLoss / WEAK_LOSSES (Ada-GVAE / Ada-ML-VAE on image
pairs) and SemiSupervisedVaeLoss / SEMI_LOSSES (S2-beta-VAE on a few labelled images), which the reference does not have.

Two ways in:
  * ``loss(data, recon, latent_dist, is_train, storer, latent_sample=...)`` -- the reference
    signature (losses.py:78); returns a 0-d tensor wired into autograd through thin
    torch.autograd.Function wrappers around the kernels, so the reference's own
    Trainer / Evaluator code keeps working with the native model;
  * ``loss.fused_step(data, model, optimizer, storer)`` -- what the native Trainer uses: one
    stream of kernel launches for forward + loss + backward (no autograd graph, gradients
    land in the flat arena, all scalars in one small device buffer), then optimizer.step().
Host-side state (n_train_steps, annealing, storer cadence) follows losses.py:71-75,105-114.
"""
import abc
import contextlib
import ctypes

import torch

from .. import _diplib
from .. import _mmdlib
from .. import _weaklib
from .. import _semilib
from .. import _lib
from .. import optim
from .._lib import call, ptr, record_py
from ..utils.math import log_importance_weights
from .discriminator import Discriminator
from ..graph import StepGraphs
from ..parallel import scale_, copy_flat_
from .._debug import knob
from ..schedule import build_policy, replay_mode, switches

LOSSES = ["VAE", "betaH", "betaB", "factor", "btcvae"]  # losses.py:17
RECON_DIST = ["bernoulli", "laplace", "gaussian"]        # losses.py:18
DIP_LOSSES = ["dipI", "dipII"]                           # DIP-VAE-I / II (Kumar et al. 2018): not in the reference, so not in LOSSES
INFO_LOSSES = ["infovae"]                                # InfoVAE / MMD-VAE (Zhao et al. 2019): not in the reference either
WEAK_LOSSES = ["adagvae", "adamlvae"]                    # Ada-GVAE / Ada-ML-VAE on image pairs (Locatello et al. 2020): nor these
SEMI_LOSSES = ["s2vae"]                                  # S2-beta-VAE on a few labelled images (Locatello et al. 2020, "Few Labels"): nor this


def get_loss_f(loss_name, **kwargs_parse):
    """losses.py:22-49 -- same keys consumed."""
    kwargs_all = dict(rec_dist=kwargs_parse["rec_dist"], steps_anneal=kwargs_parse["reg_anneal"])
    if loss_name == "betaH":
        return BetaHLoss(beta=kwargs_parse["betaH_B"], **kwargs_all)
    elif loss_name == "VAE":
        return BetaHLoss(beta=1, **kwargs_all)
    elif loss_name == "betaB":
        return BetaBLoss(C_init=kwargs_parse["betaB_initC"], C_fin=kwargs_parse["betaB_finC"],
                         gamma=kwargs_parse["betaB_G"], **kwargs_all)
    elif loss_name == "factor":
        return FactorKLoss(kwargs_parse["device"], gamma=kwargs_parse["factor_G"],
                           disc_kwargs=dict(latent_dim=kwargs_parse["latent_dim"]),
                           optim_kwargs=dict(lr=kwargs_parse["lr_disc"], betas=(0.5, 0.9)), **kwargs_all)
    elif loss_name == "btcvae":
        return BtcvaeLoss(kwargs_parse["n_data"], alpha=kwargs_parse["btcvae_A"], beta=kwargs_parse["btcvae_B"],
                          gamma=kwargs_parse["btcvae_G"], **kwargs_all)
    elif loss_name in DIP_LOSSES:
        return DipVaeLoss(dip_type="i" if loss_name == "dipI" else "ii", lambda_od=kwargs_parse.get("dip_lambda_od", 10.),
                          lambda_d_factor=kwargs_parse.get("dip_lambda_d_factor"), **kwargs_all)
    elif loss_name in INFO_LOSSES:
        return InfoVaeLoss(alpha=kwargs_parse.get("info_alpha", 0.), lam=kwargs_parse.get("info_lambda", 1000.),
                           kernel=kwargs_parse.get("mmd_kernel", "imq"), bandwidth=kwargs_parse.get("mmd_bandwidth"), **kwargs_all)
    elif loss_name in WEAK_LOSSES:
        return WeakVaeLoss(aggregation="gvae" if loss_name == "adagvae" else "mlvae", beta=kwargs_parse.get("weak_beta", 1),
                           **kwargs_all)
    elif loss_name in SEMI_LOSSES:
        return SemiSupervisedVaeLoss(lat_sizes=kwargs_parse["lat_sizes"], sup_loss=kwargs_parse.get("sup_loss", "xent"),
                                     gamma_sup=kwargs_parse.get("gamma_sup", 1.), beta=kwargs_parse.get("s2_beta", 4),
                                     sup_reduction=kwargs_parse.get("sup_reduction", "sum"),
                                     sup_anneal=kwargs_parse.get("sup_anneal", "fixed"),
                                     sup_anneal_steps=kwargs_parse.get("sup_anneal_steps", 0),
                                     sup_factors=kwargs_parse.get("sup_factors"), latent_dim=kwargs_parse.get("latent_dim"),
                                     n_data=kwargs_parse.get("n_data"), **kwargs_all)
    else:
        assert loss_name not in LOSSES
        raise ValueError("Uknown loss : {}".format(loss_name))


def linear_annealing(init, fin, step, annealing_steps):
    """losses.py:511-518."""
    if annealing_steps == 0:
        return fin
    assert fin > init
    delta = fin - init
    return min(init + delta * step / annealing_steps, fin)


from ..engine import _stream  # noqa: E402


class _Scratch:
    """Small device buffers shared by the loss kernels of one loss object."""

    def __init__(self, device):
        _lib.note_alloc()
        f = lambda n: torch.zeros(n, dtype=torch.float32, device=device)
        self.device = device
        self.coef = f(_lib.NCOEF)
        self.coef_host = [0.0] * _lib.NCOEF
        self.scal = f(_lib.NSCAL)
        self.packed = f(_lib.NPACK)
        self.partials = f(_lib.REC_NPART)
        self.kl_dim = f(_lib.KL_FLOATS)   # DVAE_KL_FLOATS: per-dim KL + per-workgroup partial blocks
        self.disc_sums = f(4)
        self.log_w = f(4)
        self._log_w_key = None
        self.rowstats = None
        self.lat = {}

    def for_latent_dim(self, D):
        """`scal` / `packed` sized for latent dimension D (include/dvae_hip.h: above DVAE_MAX_D the per-dimension KL values follow
        the 32 fixed slots) -- grown once; recorded launch plans are invalidated with the allocation."""
        if self.scal.numel() < _lib.nscal(D):
            _lib.note_alloc()
            self.scal = torch.zeros(_lib.nscal(D), dtype=torch.float32, device=self.device)
            self.packed = torch.zeros(_lib.npack(D), dtype=torch.float32, device=self.device)
        if self.kl_dim.numel() < D:
            _lib.note_alloc()
            self.kl_dim = torch.zeros(D, dtype=torch.float32, device=self.device)
        return self

    def set_coef(self, **kw):
        h = self.coef_host
        for k, v in kw.items():
            h[getattr(_lib, "C_" + k)] = float(v)
        # values travel as kernel arguments: ordered with the stream, no host sync
        call("dvae_set_coef", ptr(self.coef), *h, _stream())

    def set_coef_host(self, **kw):
        """Host copy only: the values reach the device with the step's weight-staging launch (engine.stage)."""
        h = self.coef_host
        for k, v in kw.items():
            h[getattr(_lib, "C_" + k)] = float(v)

    def set_log_w(self, batch, n_data):
        key = (batch, n_data)
        if key != self._log_w_key:
            self.log_w[:3].copy_(log_importance_weights(batch, n_data))
            self._log_w_key = key

    def latent(self, name, rows, cols):
        t = self.lat.get((name, rows, cols))
        if t is None:
            _lib.note_alloc()
            t = torch.empty(rows, cols, dtype=torch.float32, device=self.device)
            self.lat[(name, rows, cols)] = t
        return t


class BaseLoss(abc.ABC):
    """losses.py:53-114."""

    def __init__(self, record_loss_every=50, rec_dist="bernoulli", steps_anneal=0):
        self.n_train_steps = 0
        self.record_loss_every = record_loss_every
        self.rec_dist = rec_dist
        self.steps_anneal = steps_anneal
        self._scratch = None
        self.comm = None   # set by disvae_amd.parallel.data_parallel for sharded batches
        # sharded batches: "global" = the B x B estimator / permute_dims couple the GLOBAL batch (equal to the
        # single-process step on the concatenated batch); "local" = every rank's shard is its own minibatch
        # (what running the reference under DistributedDataParallel would compute: a different estimator)
        self.estimator = "global"
        # how the device side of the native training iteration is issued: None (eager) / "plan" / "graph" / "auto"
        # (schedule.replay_mode resolves it per step; read at construction: tests and bench.py assign it afterwards)
        mode = knob("DVAE_REPLAY", "auto")
        if mode not in ("plan", "graph", "eager", "auto"):
            raise ValueError("DVAE_REPLAY={!r}: expected one of auto, eager, plan, graph".format(mode))
        self.replay = {"plan": "plan", "graph": "graph", "eager": None, "auto": "auto"}[mode]
        self._graphs = StepGraphs()
        self._static = {}
        self.policy_override = {}   # StepPolicy fields forced to a value (tests: an A/B partner without the environment)
        # dvae_event_record / dvae_event_wait slot of this loss object: "the estimator and the scalar loss of this step are final"
        self._ev_slot = _lib.next_event_slot()

    def _static_buf(self, name, like):
        """Persistent device buffer with the shape/dtype of `like`, refreshed with its contents."""
        key = (name, tuple(like.shape), like.dtype)
        t = self._static.get(key)
        if t is None:
            _lib.note_alloc()
            t = self._static[key] = torch.empty(like.shape, dtype=like.dtype, device=self._scratch.device)
        if t.data_ptr() != like.data_ptr():
            t.copy_(like, non_blocking=True)
        return t

    def _begin_step(self, model, data):
        """This step's schedule.StepPolicy (built once per distinct step shape), handed to the engine."""
        pol = build_policy(model.img_size, model.latent_dim, data.shape[0], switches(), self._world()[0], self.KIND,
                           model.training, self.replay)
        if self.policy_override:
            pol = pol._replace(**self.policy_override)
        model.engine.begin_step(pol)
        return pol

    def _replay_mode(self, is_train, data):
        return replay_mode(self.replay, is_train, data.numel())

    def _replay_key(self, model, data, injected, pol):
        """Everything a recorded launch freezes: buffers (allocation generation), arenas, the batch pointer, the stream, the
        step's policy (every scheduling decision) and the few Python-side switches passed as scalars."""
        return (id(model), data.shape, data.data_ptr(), injected, _stream(), model.arena.flat.data_ptr(),
                model.arena.grad.data_ptr(), _lib.ALLOC_GEN[0], self.rec_dist, getattr(self, "is_mss", None), pol,
                id(self.comm), self.estimator)

    @abc.abstractmethod
    def __call__(self, data, recon_data, latent_dist, is_train, storer, **kwargs):
        pass

    def _pre_call(self, is_train, storer):
        if is_train:
            self.n_train_steps += 1
        if not is_train or self.n_train_steps % self.record_loss_every == 1:
            return storer
        return None

    def scratch(self, device):
        if self._scratch is None or self._scratch.device != device:
            self._scratch = _Scratch(device)
        return self._scratch

    def _pack_sums(self, sc, klb, D, rowstats, Bl, disc_sums, packed, stream):
        """This rank's partial sums -> `packed` (sharded batches: sum-all-reduced over the ranks before dvae_loss_finalize) in
        ONE launch: dvae_loss_epilogue without `scal` is dvae_kl_finish (the klb KL partial blocks the fused FC chain left) +
        dvae_loss_pack, bit for bit (tests/test_gpu_kernels.py::test_loss_epilogue_equals_pack_then_finalize) -- one dependent
        launch less on the exchange stream, which the FC chain's input gradients wait for."""
        call("dvae_loss_epilogue", _lib.LOSS_BETAH, ptr(sc.partials), ptr(sc.kl_dim), klb, D, ptr(rowstats), Bl, ptr(disc_sums), 1,
             ptr(sc.coef), ptr(packed), None, stream)

    def _rec_code(self):
        if self.rec_dist not in _lib.REC:
            assert self.rec_dist not in RECON_DIST
            raise ValueError("Unkown distribution: {}".format(self.rec_dist))  # losses.py:442
        return _lib.REC[self.rec_dist]

    # world size / rank of the data-parallel group (1 / 0 without a communicator)
    def _world(self):
        return (1, 0) if self.comm is None else (self.comm.world_size, self.comm.rank)

    def _est_world(self):
        """(world, rank) as seen by the batch-coupled estimators."""
        return (1, 0) if (self.comm is None or self.estimator == "local") else (self.comm.world_size, self.comm.rank)

    # what a step logs, in this order: (storer key, scalar slot); 'kl_loss' brings the per-dimension values with it
    STORED = ()

    def _store(self, storer, sc, D, keys=None):
        if storer is None:
            return
        vals = sc.scal.tolist()           # ONE device->host copy for every logged scalar
        for key, slot in self.STORED if keys is None else keys:
            if key == 'kl_loss':
                self._store_kl(storer, vals, D)
            else:
                storer[key].append(vals[slot])

    @staticmethod
    def _store_kl(storer, vals, D):
        storer['kl_loss'].append(vals[_lib.S_KL])
        for i in range(D):
            storer['kl_loss_' + str(i)].append(vals[_lib.kl0(D) + i])

    # ---- the parts of a native step (the skeleton: DESIGN.md, "The step skeleton") ---------------------------------------
    def _run_step(self, model, data, pol, inputs, injected, key_extra, fn):
        """Replay dispatch: fn(data, *inputs) now, or recorded / replayed (graph.py).  A replay re-issues launches with frozen
        pointers: the injected `inputs` [(name, tensor or None)] go through static buffers; the batch pointer is part of the plan
        key (a hipGraph needs it static as well)."""
        mode = pol.replay
        if not mode:
            return fn(data, *[t for _, t in inputs])
        if mode == "graph":
            data = self._static_buf("data", data)
        inputs = [t if t is None else self._static_buf(name, t) for name, t in inputs]
        self._graphs.run(self._replay_key(model, data, injected, pol) + key_extra, lambda: fn(data, *inputs), mode)

    def _finish_loss(self, sc, klb, D, rowstats, rows, disc_sums, Bg, stream, on=None, xbuf=None):
        """The scalar epilogue on `stream`: partial sums -> sc.scal.  Single process: ONE launch.  Sharded: pack, sum-all-reduce
        over the ranks (issued under torch stream `on`, the handle of `stream`, when that is not the current one), finalize; with
        `xbuf` (the sharded beta-TCVAE estimator's column gradients) the sums are packed behind them and ride in their
        collective."""
        if self.comm is None or self.comm.world_size == 1:
            call("dvae_loss_epilogue", self.KIND, ptr(sc.partials), ptr(sc.kl_dim), klb, D, ptr(rowstats), rows, ptr(disc_sums), Bg,
                 ptr(sc.coef), ptr(sc.packed), ptr(sc.scal), stream)
            return
        npk = _lib.npack(D)
        packed = sc.packed if xbuf is None else xbuf[xbuf.numel() - npk:]
        self._pack_sums(sc, klb, D, rowstats, rows, disc_sums, packed, stream)
        with contextlib.nullcontext() if on is None else torch.cuda.stream(on):
            if xbuf is None:
                self.comm.all_reduce(packed)
            else:                                 # + the estimator's column gradients: one collective
                self.comm.all_reduce_cols_sums(xbuf, rows, D, npk)
        call("dvae_loss_finalize", self.KIND, ptr(packed), D, Bg, ptr(sc.coef), ptr(sc.scal), stream)

    def _defer_loss(self, eng, finish):
        """The late join.  Nothing on the current stream needs the scalar loss (or the beta-TCVAE estimator) before the FC chain's
        input gradients, a whole convT backward later -- joining earlier left this stream idle for ~20 us plus the epilogue
        (profiles/r04_v35_btcvae_celeba_timeline.md).  `finish(stream, on)` therefore runs behind the NEXT fork (the backward
        pass's first: no fork of its own) on the side stream -- sharded, on the exchange stream behind the estimator, ordered
        after the fork point through the side stream (whose only queued work at that moment is the wait for that fork: no second
        event on this stream) -- and an event slot marks the lot.  Returns what fc_chain() calls first: the wait for the slot."""
        s = _stream()
        sharded = eng.policy.sharded

        def deferred():
            ss = eng._side_raw()
            if sharded:
                ss = eng._aux_raw()
                call("dvae_stream_order", eng._side_raw(), ss)
            finish(ss, eng.aux_stream if sharded else None)
            call("dvae_event_record", self._ev_slot, ss)
        eng.at_next_fork(deferred)

        def wait():
            eng.flush_fork_hook()
            call("dvae_event_wait", self._ev_slot, s)
        return wait

    def _backward(self, eng, model, data, buf, n, fc_chain, pending=()):
        """Both backward passes and the gradient exchange; one join, at the end of encode_backward.  Single process: ONE grouped
        launch for all six FC weight gradients (issued by encode_backward).  Sharded, two spans: the decoder's three are launched
        with the decoder's conv weight gradients -- every kernel that writes a decoder gradient goes to the side stream, so the
        all-reduce of the decoder span is ordered behind the SIDE stream and overlaps the encoder backward; this stream never
        waits for it before the end.  Without spans (schedule.SMALL_SHARD_ELEMS): ONE all-reduce of the whole arena after the join.
        pending: handles of collectives already under way (FactorVAE: the discriminator's gradients), waited for last."""
        spans = eng.policy.grad_spans
        pending = list(pending)
        dec_fc = eng.decode_backward(buf.z, buf, n=n, join=False, defer_fc_wgrad=not spans, fc_chain=fc_chain)
        if spans:
            with torch.cuda.stream(eng.side_stream):
                pending.append(self.comm.all_reduce_async(model.arena.span("decoder.")))
        eng.encode_backward(data, buf, n=n, fc_chain=True, dec_fc=dec_fc)
        if spans:
            pending.append(self.comm.all_reduce_async(model.arena.span("encoder.")))
        elif eng.policy.sharded:
            self.comm.all_reduce(model.arena.grad)
        for h_ in pending:
            h_.wait()


# ------------------------------------------------------------------------------------------
# autograd-compatible pieces (reference call signature)
# ------------------------------------------------------------------------------------------
class _ReconLossFn(torch.autograd.Function):
    """_reconstruction_loss (losses.py:394-449): sum over pixels / batch."""

    @staticmethod
    def forward(ctx, recon, data, dist_code, scratch):
        recon, data = recon.contiguous(), data.contiguous()
        B = recon.shape[0]
        scratch.set_coef(INV_B=1.0 / B)
        g = torch.empty_like(recon)
        call("dvae_recon_loss", ptr(recon), ptr(data), recon.numel(), dist_code, ptr(scratch.coef),
             ptr(scratch.partials), ptr(g), 0, _stream())
        ctx.save_for_backward(g)
        out = torch.empty((), dtype=torch.float32, device=recon.device)
        call("dvae_reduce_sum", ptr(scratch.partials), _lib.REC_NPART, 1.0 / B, ptr(out), _stream())
        return out

    @staticmethod
    def backward(ctx, gout):
        (g,) = ctx.saved_tensors
        return g * gout, None, None, None


class _KLFn(torch.autograd.Function):
    """_kl_normal_loss (losses.py:452-480) -> per-dim KL [D] (mean over batch)."""

    @staticmethod
    def forward(ctx, mu, logvar, scratch):
        B, D = mu.shape
        ml = torch.stack((mu, logvar), dim=-1).reshape(B, 2 * D).contiguous()
        scratch.set_coef(INV_B=1.0 / B)
        tmp = torch.empty(3, B, D, dtype=torch.float32, device=mu.device)
        kl_dim = torch.empty(max(16 + 64 * 16, D), dtype=torch.float32, device=mu.device)
        call("dvae_reparam_kl_fwd", ptr(ml), None, ptr(tmp[0]), ptr(tmp[1]), ptr(tmp[2]), ptr(kl_dim),
             ptr(scratch.coef), B, D, _stream())
        ctx.save_for_backward(mu, logvar)
        return kl_dim[:D].clone()

    @staticmethod
    def backward(ctx, gout):
        mu, logvar = ctx.saved_tensors
        B, D = mu.shape
        mu, logvar, gout = mu.contiguous(), logvar.contiguous(), gout.contiguous()
        gmu, glv = torch.empty_like(mu), torch.empty_like(logvar)
        call("dvae_kl_normal_bwd", ptr(gout), ptr(mu), ptr(logvar), ptr(gmu), ptr(glv), B, D, _stream())
        return gmu, glv, None


class _BtcvaeFn(torch.autograd.Function):
    """_get_log_pz_qz_prodzi_qzCx + the three batch means (losses.py:364-373, 523-544) ->
    tensor [mi, tc, dw_kl]; backward through dvae_btcvae_bwd for each requested term."""

    @staticmethod
    def forward(ctx, z, mu, logvar, n_data, is_mss, scratch):
        z, mu, logvar = z.contiguous(), mu.contiguous(), logvar.contiguous()
        B, D = z.shape
        scratch.set_log_w(B, n_data)
        rowstats = torch.empty(B, _lib.rowstats_stride(D), dtype=torch.float32, device=z.device)
        tmp = torch.empty(_lib.btcvae_tmp_floats(B, B, D), dtype=torch.float32, device=z.device)
        call("dvae_btcvae_fwd", ptr(z), ptr(mu), ptr(logvar), B, D, 0, B, int(is_mss), ptr(scratch.log_w),
             ptr(tmp), ptr(rowstats), _stream())
        # batch means of the four log-densities -> (mi, tc, dw_kl) by the scalar epilogue kernels (losses.py:369-373); no KL
        # values are passed (kl_dim = NULL): D only tells the kernels the row stride of `rowstats`
        packed = torch.empty(_lib.npack(D), dtype=torch.float32, device=z.device)
        scal = torch.empty(_lib.nscal(D), dtype=torch.float32, device=z.device)
        call("dvae_loss_pack", ptr(scratch.partials), None, D, ptr(rowstats), B, None, ptr(packed), _stream())
        call("dvae_loss_finalize", _lib.LOSS_BTCVAE, ptr(packed), D, B, ptr(scratch.coef), ptr(scal), _stream())
        ctx.save_for_backward(z, mu, logvar, rowstats, tmp)
        ctx.is_mss, ctx.scratch = is_mss, scratch
        return scal[_lib.S_MI:_lib.S_DWKL + 1].clone()       # [mi, tc, dw_kl]

    @staticmethod
    def backward(ctx, gout):
        z, mu, logvar, rowstats, tmp = ctx.saved_tensors
        B, D = z.shape
        # d(a*mi + b*tc + c*dw)/d(.) with (alpha, beta, gamma*anneal) = (a, b, c)
        a, b, c = [float(v) for v in gout.tolist()]
        coef = torch.zeros(_lib.NCOEF, dtype=torch.float32)
        coef[_lib.C_ALPHA], coef[_lib.C_BETA], coef[_lib.C_GAMMA], coef[_lib.C_ANNEAL] = a, b, c, 1.0
        coef = coef.to(z.device)
        dz, dmu, dlv = torch.empty_like(z), torch.empty_like(z), torch.empty_like(z)
        call("dvae_btcvae_bwd", ptr(z), ptr(mu), ptr(logvar), ptr(rowstats), B, D, 0, B, int(ctx.is_mss),
             ptr(ctx.scratch.log_w), ptr(coef), ptr(tmp), ptr(dz), ptr(dmu), ptr(dlv), _stream())
        return dz, dmu, dlv, None, None, None


def _dip_launches(mu, logvar, lambda_od, lambda_d, ws, dmu, dlv, out, loss_io, stream):
    """The two launches of libdvae_dip_hip.so (include/dvae_dip_hip.h) on a [B, D] batch; logvar None: DIP-VAE-I.  Through
    record_py: a recorded plan re-issues them with these arguments, a hipGraph captures them."""
    B, D = mu.shape
    record_py(_diplib.call, "dvae_dip_moments", ptr(mu), ptr(logvar), B, D, ptr(ws), stream)
    record_py(_diplib.call, "dvae_dip_grad", ptr(mu), ptr(logvar), B, D, float(lambda_od), float(lambda_d), ptr(ws), ptr(dmu),
              ptr(dlv), ptr(out), loss_io, stream)


class _DipFn(torch.autograd.Function):
    """The DIP-VAE regulariser R(mu, logvar) (logvar None: type I) -> 0-d tensor; value and both gradients come from the same
    two launches as in the fused step, so backward only scales what forward saved."""

    @staticmethod
    def forward(ctx, mu, logvar, lambda_od, lambda_d):
        mu = mu.contiguous()
        logvar = None if logvar is None else logvar.contiguous()
        B, D = mu.shape
        f64 = lambda n: torch.empty(n, dtype=torch.float64, device=mu.device)
        ws, out = f64(_diplib.ws_doubles(B, D)), f64(_diplib.out_doubles(D))
        dmu = torch.empty_like(mu)
        dlv = None if logvar is None else torch.empty_like(mu)
        _dip_launches(mu, logvar, lambda_od, lambda_d, ws, dmu, dlv, out, None, _stream())
        ctx.save_for_backward(dmu, dlv)
        return out[0].float()

    @staticmethod
    def backward(ctx, gout):
        dmu, dlv = ctx.saved_tensors
        return dmu * gout, None if dlv is None else dlv * gout, None, None


def _mmd_launches(z, prior, mu, kernel, h, w, ws, dmu, dlv, out, loss_io, stream):
    """The two launches of libdvae_mmd_hip.so (include/dvae_mmd_hip.h) on a [B, D] batch of latent samples and as many prior
    draws; dmu None: the value only.  Through record_py: a recorded plan re-issues them with these arguments, a hipGraph captures
    them."""
    B, D = z.shape
    record_py(_mmdlib.call, "dvae_mmd_pairs", ptr(z), ptr(prior), B, D, _mmdlib.KERNELS[kernel], float(h), int(dmu is not None),
              ptr(ws), stream)
    record_py(_mmdlib.call, "dvae_mmd_finish", ptr(z), ptr(mu), B, D, float(w), ptr(ws), ptr(dmu), ptr(dlv), ptr(out), loss_io,
              stream)


class _MmdFn(torch.autograd.Function):
    """w MMD_u(z, prior) -> 0-d tensor; the value and the gradient with respect to z come from the same two launches as in the
    fused step, so backward only scales what forward saved."""

    @staticmethod
    def forward(ctx, z, prior, kernel, h, w):
        z, prior = z.contiguous(), prior.contiguous()
        B, D = z.shape
        f64 = lambda n: torch.empty(n, dtype=torch.float64, device=z.device)
        ws, out = f64(_mmdlib.ws_doubles(B, D)), f64(_mmdlib.OUT_DOUBLES)
        dz = torch.empty_like(z)
        _mmd_launches(z, prior, None, kernel, h, w, ws, dz, None, out, None, _stream())
        ctx.save_for_backward(dz)
        return out[0].float()

    @staticmethod
    def backward(ctx, gout):
        (dz,) = ctx.saved_tensors
        return dz * gout, None, None, None, None


def _semi_launches(mu, rows, K, table, kind, reduction, w_ptr, ws, dmu, out, loss_io, stream):
    """The two launches of libdvae_semi_hip.so (include/dvae_semi_hip.h) on a split [n, D] batch of posterior means and its row
    numbers (negative: unlabelled); table: the (sizes, strides) ctypes arrays of _semilib.factor_table, whose host addresses the
    calls take; w_ptr: the DEVICE address of the term's weight; dmu None: the value only.  Through record_py: a recorded plan
    re-issues them with these arguments, a hipGraph captures them."""
    n, D = mu.shape
    sizes, strides = ctypes.addressof(table[0]), ctypes.addressof(table[1])
    record_py(_semilib.call, "dvae_semi_partials", ptr(mu), 0, ptr(rows), n, D, K, sizes, strides, kind, ptr(ws), stream)
    record_py(_semilib.call, "dvae_semi_grad", ptr(mu), 0, ptr(rows), n, D, K, sizes, strides, kind, reduction, w_ptr, ptr(ws),
              ptr(dmu), ptr(out), loss_io, stream)


class _SemiFn(torch.autograd.Function):
    """The supervised regulariser R_sup(mu, rows) of SemiSupervisedVaeLoss (weight 1) -> 0-d tensor; the value and the gradient
    come from the same two launches as in the fused step, so backward only scales what forward saved."""

    @staticmethod
    def forward(ctx, mu, rows, K, table, kind, reduction):
        mu, rows = mu.contiguous(), rows.contiguous()
        n, D = mu.shape
        f64 = lambda m: torch.empty(m, dtype=torch.float64, device=mu.device)
        ws, out = f64(_semilib.ws_doubles(n, D, K)), f64(_semilib.out_doubles(D, K))
        one = torch.ones(1, dtype=torch.float32, device=mu.device)
        dmu = torch.empty_like(mu)
        _semi_launches(mu, rows, K, table, kind, reduction, ptr(one), ws, dmu, out, None, _stream())
        ctx.save_for_backward(dmu)
        return out[0].float()

    @staticmethod
    def backward(ctx, gout):
        (dmu,) = ctx.saved_tensors
        return dmu * gout, None, None, None, None, None


class _PairAggregate:
    """The latent operator of the pair losses as VAEEngine._fc_layers_fwd / _fc_layers_bwd take it: the two launches of
    libdvae_weak_hip.so (include/dvae_weak_hip.h) around the reparameterisation, on the interleaved [rows, 2 D] layout; rows i and
    rows / 2 + i are a pair.  Through record_py: a recorded plan re-issues them with these arguments, a hipGraph captures them."""

    def __init__(self, kind, D, ml_agg, shared, delta, stream):
        self.kind, self.D, self.ml_agg, self.shared, self.delta, self.stream = kind, D, ml_agg, shared, delta, stream

    def fwd(self, ml, rows):
        record_py(_weaklib.call, "dvae_weak_aggregate_fwd", ptr(ml), rows // 2, self.D, self.kind, ptr(self.ml_agg),
                  ptr(self.shared), ptr(self.delta), self.stream)
        return self.ml_agg

    def bwd(self, ml, dml, rows):
        record_py(_weaklib.call, "dvae_weak_aggregate_bwd", ptr(ml), ptr(self.shared), rows // 2, self.D, self.kind, ptr(dml),
                  self.stream)


def _check_pairs(rows, D):
    """What a batch of pairs has to satisfy, before any device work."""
    if rows < 2 or rows % 2:
        raise ValueError("a batch of pairs has an even number of rows (rows i and rows / 2 + i are a pair), got {}".format(rows))
    if not 1 <= D <= _weaklib.MAX_D:
        raise ValueError("the pair losses take 1 <= latent_dim <= {} (the mask of a pair is one 64-bit word), got {}".format(
            _weaklib.MAX_D, D))


def _interleave(a, b):
    """[B, D] x 2 -> the interleaved [B, 2 D] layout of mu_logvar_gen, contiguous and owned."""
    return torch.stack((a, b), dim=-1).reshape(a.shape[0], 2 * a.shape[1]).contiguous()


class _AdaptiveGroupFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mu, logvar, kind):
        B, D = mu.shape
        ml = _interleave(mu.float(), logvar.float())
        ml_agg = torch.empty_like(ml)
        shared = torch.empty(B // 2, dtype=torch.int64, device=mu.device)
        op = _PairAggregate(kind, D, ml_agg, shared, None, _stream())
        op.fwd(ml, B)
        ctx.save_for_backward(ml, shared)
        ctx.kind = kind
        ctx.mark_non_differentiable(shared)
        return ml_agg[:, 0::2].contiguous(), ml_agg[:, 1::2].contiguous(), shared

    @staticmethod
    def backward(ctx, gmu, glv, _gshared):
        ml, shared = ctx.saved_tensors
        B, D = ml.shape[0], ml.shape[1] // 2
        zero = lambda g: torch.zeros(B, D, dtype=torch.float32, device=ml.device) if g is None else g.float()
        dml = _interleave(zero(gmu), zero(glv))
        _PairAggregate(ctx.kind, D, None, shared, None, _stream()).bwd(ml, dml, B)
        return dml[:, 0::2], dml[:, 1::2], None


def adaptive_group_posterior(mu, logvar, aggregation="gvae"):
    """The adaptive group posterior of Ada-GVAE ("gvae") / Ada-ML-VAE ("mlvae") (Locatello et al. 2020) of a batch of pairs:
    mu, logvar fp32 [2 P, D] device tensors, rows i and P + i a pair -> (mu~, logvar~, shared): the aggregated posterior
    parameters [2 P, D] (a dimension that the pair shares -- delta < tau, include/dvae_weak_hip.h -- holds the same bits in both
    rows, every other element is its input) and the mask, int64 [P] with bit d set where dimension d is shared.  Differentiable
    with respect to mu and logvar through the library's backward launch; the mask is a constant.  For models that are not the
    engine's: WeakVaeLoss.fused_step runs the same two launches inside the native step."""
    if aggregation not in _weaklib.KINDS:
        raise ValueError("aggregation must be one of {}, got {!r}".format(sorted(_weaklib.KINDS), aggregation))
    if mu.dim() != 2 or mu.shape != logvar.shape:
        raise ValueError("mu and logvar must be [2 P, D] tensors of one shape, got {} and {}".format(tuple(mu.shape),
                                                                                                     tuple(logvar.shape)))
    _check_pairs(mu.shape[0], mu.shape[1])
    return _AdaptiveGroupFn.apply(mu, logvar, _weaklib.KINDS[aggregation])


def popcount64(words):
    """Set bits of each element of an int64 tensor (the pair masks), on the host -> int64 [n]."""
    w = words.detach().cpu().contiguous().view(-1)
    n = torch.zeros_like(w)
    for k in range(64):
        n += (w >> k) & 1
    return n


def u8_to_f32(x):
    """ToTensor's arithmetic on a uint8 device tensor: float(v) / 255 (dvae_u8_to_f32)."""
    x = x.contiguous()
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    call("dvae_u8_to_f32", ptr(x), ptr(out), x.numel(), _stream())
    return out


def _reconstruction_loss(data, recon_data, distribution="bernoulli", storer=None, scratch=None):
    """losses.py:394-449."""
    if distribution not in _lib.REC:
        assert distribution not in RECON_DIST
        raise ValueError("Unkown distribution: {}".format(distribution))
    scratch = scratch or _Scratch(recon_data.device)
    if data.dtype == torch.uint8:              # pixel batches: ToTensor (utils/datasets.py:207-209) on the device
        data = u8_to_f32(data)
    loss = _ReconLossFn.apply(recon_data, data, _lib.REC[distribution], scratch)
    if distribution == "laplace":
        loss = loss * (loss != 0)
    if storer is not None:
        storer['recon_loss'].append(loss.item())
    return loss


def _kl_normal_loss(mean, logvar, storer=None, scratch=None):
    """losses.py:452-480."""
    scratch = scratch or _Scratch(mean.device)
    latent_kl = _KLFn.apply(mean, logvar, scratch)
    total_kl = latent_kl.sum()
    if storer is not None:
        storer['kl_loss'].append(total_kl.item())
        for i in range(mean.size(1)):
            storer['kl_loss_' + str(i)].append(latent_kl[i].item())
    return total_kl


def _permute_dims(latent_sample, perms=None):
    """losses.py:483-508; the permutations are drawn with torch.randperm on the CPU generator
    like the reference (:505) unless injected (perms: int64 [D,B])."""
    B, D = latent_sample.shape
    if perms is None:
        perms = torch.stack([torch.randperm(B) for _ in range(D)])
    perms = perms.to(device=latent_sample.device, dtype=torch.int64).contiguous()
    out = torch.empty_like(latent_sample)
    call("dvae_permute_dims", ptr(latent_sample.contiguous()), ptr(perms), ptr(out), B, D, _stream())
    return out


# ------------------------------------------------------------------------------------------
# loss classes
# ------------------------------------------------------------------------------------------
class _SingleOptimizerLoss(BaseLoss):
    """Shared fused step of BetaH / BetaB / Btcvae (training.py:152-158 + the loss __call__)."""

    KIND = None
    STORED = (('recon_loss', _lib.S_REC), ('kl_loss', _lib.S_KL), ('loss', _lib.S_LOSS))

    def _coefs(self, is_train):
        raise NotImplementedError

    def _regulariser(self, buf, sc, B, D, is_train, stream, *noise):
        """Hook of _device_step: launches on `stream` behind the loss epilogue that add a term to sc.scal[S_LOSS] -> its
        (dmu_x, dlv_x) for the FC chain's backward pass (None: no such term, no launch).  Only for steps whose epilogue is not
        deferred (StepPolicy.late_join: beta-TCVAE and sharded steps), or the term would be added before the epilogue writes.
        noise: the tensors (or None: draw) of fused_step's `extra_noise`, in its order."""
        return None

    def fused_step(self, data, model, optimizer, storer, eps=None, extra_noise=()):
        """extra_noise: [(name, tensor or None)] -- injectable noise of a regulariser hook beyond eps (InfoVaeLoss: the prior
        draws); it goes through _run_step's static buffers exactly as eps does and reaches _regulariser.  Empty for every
        other loss: their inputs, launch order and draw order are what they were."""
        is_train = model.training
        storer = self._pre_call(is_train, storer)
        B, D = data.shape[0], model.latent_dim
        sc = self.scratch(data.device).for_latent_dim(D)
        # ONE launch: this step's weight images (32-channel conv layers, FC chain) + its loss coefficients
        sc.set_coef_host(INV_B=1.0 / (B * self._world()[0]), **self._coefs(is_train))
        model.engine.stage(sc.coef, sc.coef_host)
        data = data.contiguous()
        pol = self._begin_step(model, data)
        if self.KIND == _lib.LOSS_BTCVAE:
            sc.set_log_w(B * self._est_world()[0], self.n_data)
        inputs = [("eps", eps)] + list(extra_noise)
        self._run_step(model, data, pol, inputs, any(t is not None for _, t in inputs), (),
                       lambda data, eps, *noise: self._device_step(data, model, sc, eps, is_train, *noise))
        if is_train:
            model.assign_grads()          # optimizer.zero_grad(); loss.backward()  (training.py:156-157)
            optim.step(optimizer)         # optimizer.step(), training.py:158 (one launch for a stock Adam: disvae_amd/optim.py)
        self._store(storer, sc, D)
        return sc.scal[_lib.S_LOSS]

    def _device_step(self, data, model, sc, eps, is_train, *noise):
        """Forward + loss + backward as one stream of launches; no host-dependent values."""
        eng = model.engine
        B, D = data.shape[0], model.latent_dim
        world = self._world()[0]
        Bg = B * world
        buf = eng.buffers(B)
        s = _stream()
        data = eng.input(data, buf)            # uint8 pixel batches: fused /255 (or one ToTensor pass), see engine.input
        if is_train and eps is None:
            eps = sc.latent("eps", B, D)
            record_py(eps.normal_)             # = torch.randn_like (vae.py:67): same Philox consumption
        if not is_train:
            eps = None
        ends = eng.encode_convs(data, buf, chain=True)
        # the FC core in one launch: lin1 -> lin2 -> mu_logvar -> reparameterise (+ KL partial blocks) -> lin1 -> lin2 -> lin3
        # (latent dimensions above 16: one launch per layer, kl_dim final at once and klb = 0 -- engine.fc_chain_fwd)
        eng.fc_chain_fwd(buf, eps, sc.kl_dim, B, coef=sc.coef, ends=ends)
        klb = eng.kl_blocks(B)            # single process: the one-launch loss epilogue finishes the KL partials
        btc = self.KIND == _lib.LOSS_BTCVAE
        rowstats = dz = dmu = dlv = xbuf = None
        if btc and world == 1:
            # the B x B estimator on the side stream while the decoder forward occupies the current one
            eng.fork_side()
            rowstats, dz, dmu, dlv, xbuf = self._estimator(eng, buf, sc, B, D, is_train)
        elif btc:
            # sharded: the estimator with its exchanges on a stream of its own (engine.buffers: the side stream is the tail of
            # the iteration, nothing may queue in front of its weight gradients)
            call("dvae_stream_order", s, eng._aux_raw())
        # decoder convT stack; its last layer also evaluates the reconstruction likelihood and dL/dlogit
        eng.decode_convs(buf, B, fuse_loss=(data, self._rec_code(), sc.coef, sc.partials), ends=ends)
        if btc and world > 1:
            # sharded: this stream's launches are issued FIRST -- the exchanges make the side stream's part long to issue, and
            # at a hundred images per GPU the host is what the critical path would wait for
            rowstats, dz, dmu, dlv, xbuf = self._estimator(eng, buf, sc, B, D, is_train)
        # the scalar epilogue: deferred behind the estimator's backward kernels, which run past the end of the decoder forward
        # (_defer_loss), for beta-TCVAE and for every sharded step (StepPolicy.late_join)
        wait = None
        if eng.policy.late_join:
            wait = self._defer_loss(eng, lambda stream, on: self._finish_loss(sc, klb, D, rowstats, B, None, Bg, stream, on, xbuf))
        else:
            if btc and world > 1:
                call("dvae_stream_order", eng._aux_raw(), s)
            elif btc:
                eng._join_side()
            self._finish_loss(sc, klb, D, rowstats, B, None, Bg, s)
        # a regulariser of the batch's (mu, logvar) or latent sample beyond the KL term (DIP-VAE, InfoVAE): its launches behind
        # the epilogue on this stream, its gradients into the FC chain like the estimator's; nothing for the reference's losses
        reg = self._regulariser(buf, sc, B, D, is_train, s, *noise)
        if reg is not None:
            assert wait is None, "a regulariser hook behind a deferred epilogue"
            dmu, dlv = reg
        if not is_train:
            return

        def fc_chain():        # the six FC input gradients + the reparameterisation / KL backward in ONE launch
            if wait is not None:
                wait()
            eng.fc_chain_bwd(buf, eps, dz, None, dmu, dlv, sc.scal, sc.coef, B)
        self._backward(eng, model, data, buf, B, fc_chain)


class BetaHLoss(_SingleOptimizerLoss):
    """losses.py:117-153."""
    KIND = _lib.LOSS_BETAH

    def __init__(self, beta=4, **kwargs):
        super().__init__(**kwargs)
        self.beta = beta

    def _coefs(self, is_train):
        anneal = linear_annealing(0, 1, self.n_train_steps, self.steps_anneal) if is_train else 1
        return dict(ANNEAL=anneal, BETA=self.beta)

    def __call__(self, data, recon_data, latent_dist, is_train, storer, **kwargs):
        storer = self._pre_call(is_train, storer)
        sc = self.scratch(recon_data.device)
        rec_loss = _reconstruction_loss(data, recon_data, storer=storer, distribution=self.rec_dist, scratch=sc)
        kl_loss = _kl_normal_loss(*latent_dist, storer, scratch=sc)
        anneal_reg = linear_annealing(0, 1, self.n_train_steps, self.steps_anneal) if is_train else 1
        loss = rec_loss + anneal_reg * (self.beta * kl_loss)
        if storer is not None:
            storer['loss'].append(loss.item())
        return loss


class DipVaeLoss(_SingleOptimizerLoss):
    """DIP-VAE-I / DIP-VAE-II (Kumar et al. 2018; disentanglement_lib's DIPVAE -- the reference has no counterpart):

        loss = rec + anneal * KL + lambda_od sum_{d != e} C_de^2 + lambda_d sum_d (C_dd - 1)^2,   lambda_d = lambda_d_factor * lambda_od

    with C the biased covariance of the batch's posterior means (type "i"), plus the diagonal of the batch mean of
    exp(logvar) (type "ii").  rec and KL are BetaHLoss's with beta = 1, and steps_anneal acts on the KL term as there; the
    regulariser is never annealed.  lambda_d_factor None: 10 for type I, 1 for type II (disentanglement_lib's defaults).
    The regulariser couples the whole batch: data-parallel steps are not built (fused_step raises under a communicator of
    more than one rank)."""
    KIND = _lib.LOSS_BETAH
    STORED = (('recon_loss', _lib.S_REC), ('kl_loss', _lib.S_KL), ('dip_loss', None), ('loss', _lib.S_LOSS))

    def __init__(self, dip_type="i", lambda_od=10., lambda_d_factor=None, **kwargs):
        super().__init__(**kwargs)
        if dip_type not in ("i", "ii"):
            raise ValueError("dip_type must be 'i' or 'ii', got {!r}".format(dip_type))
        self.dip_type = dip_type
        self.beta = 1
        self.lambda_od = float(lambda_od)
        self.lambda_d_factor = float({"i": 10., "ii": 1.}[dip_type] if lambda_d_factor is None else lambda_d_factor)
        self._dip = {}

    @property
    def lambda_d(self):
        return self.lambda_d_factor * self.lambda_od

    def _coefs(self, is_train):
        anneal = linear_annealing(0, 1, self.n_train_steps, self.steps_anneal) if is_train else 1
        return dict(ANNEAL=anneal, BETA=self.beta)

    def _dip_buf(self, device, name, n):
        """fp64 buffers of the two launches, allocated once: ("ws", B, D) the workspace, ("out", D) value and covariance."""
        t = self._dip.get((device,) + name)
        if t is None:
            _lib.note_alloc()
            t = self._dip[(device,) + name] = torch.zeros(n, dtype=torch.float64, device=device)
        return t

    def _regulariser(self, buf, sc, B, D, is_train, stream):
        """R on top of the epilogue's rec + anneal * KL in sc.scal[S_LOSS] (dvae_dip_grad's loss_io: no third launch) -> the
        gradients for the FC chain; evaluation: the value only."""
        ws = self._dip_buf(sc.device, ("ws", B, D), _diplib.ws_doubles(B, D))
        out = self._dip_buf(sc.device, ("out", D), _diplib.out_doubles(D))
        lv = buf.logvar if self.dip_type == "ii" else None
        dmu = sc.latent("dip_dmu", B, D) if is_train else None
        dlv = sc.latent("dip_dlv", B, D) if is_train and lv is not None else None
        _dip_launches(buf.mu, lv, self.lambda_od, self.lambda_d, ws, dmu, dlv, out, ptr(sc.scal) + 4 * _lib.S_LOSS, stream)
        return dmu, dlv

    def _replay_key(self, model, data, injected, pol):
        return super()._replay_key(model, data, injected, pol) + (self.lambda_od, self.lambda_d, self.dip_type)

    def _store(self, storer, sc, D, keys=None):
        if storer is None:
            return
        vals = sc.scal.tolist()
        dip = self._dip[(sc.device, "out", D)][0].item()        # fp64 [R, R_od, R_d, C]: a second small copy, on logging steps only
        for key, slot in self.STORED:
            if key == 'kl_loss':
                self._store_kl(storer, vals, D)
            else:
                storer[key].append(dip if key == 'dip_loss' else vals[slot])

    def fused_step(self, data, model, optimizer, storer, eps=None):
        if self._world()[0] > 1:
            raise NotImplementedError(
                "DIP-VAE under data parallelism is not built: the covariance couples the GLOBAL batch, so a sharded step has to "
                "gather the latents of every rank first, as the beta-TCVAE estimator does (Comm.all_gather_latents)")
        return super().fused_step(data, model, optimizer, storer, eps=eps)

    def __call__(self, data, recon_data, latent_dist, is_train, storer, **kwargs):
        storer = self._pre_call(is_train, storer)
        sc = self.scratch(recon_data.device)
        rec_loss = _reconstruction_loss(data, recon_data, storer=storer, distribution=self.rec_dist, scratch=sc)
        kl_loss = _kl_normal_loss(*latent_dist, storer, scratch=sc)
        mu, logvar = latent_dist
        dip_loss = _DipFn.apply(mu, logvar if self.dip_type == "ii" else None, self.lambda_od, self.lambda_d)
        anneal_reg = linear_annealing(0, 1, self.n_train_steps, self.steps_anneal) if is_train else 1
        loss = rec_loss + anneal_reg * (self.beta * kl_loss) + dip_loss
        if storer is not None:
            storer['dip_loss'].append(dip_loss.item())
            storer['loss'].append(loss.item())
        return loss


class InfoVaeLoss(_SingleOptimizerLoss):
    """InfoVAE (Zhao, Song & Ermon 2019; alpha = 1: MMD-VAE; the MMD term is WAE-MMD's regulariser -- the reference has no
    counterpart):

        loss = rec + anneal * (1 - alpha) * KL + (alpha + lam - 1) * MMD_u(z, p)

    rec and KL are BetaHLoss's with beta = 1 - alpha, and steps_anneal acts on the KL term as there; the MMD term is never
    annealed.  z is the batch's latent sample (in evaluation: the mean), p are B x D standard-normal draws and MMD_u is the
    unbiased U-statistic (include/dvae_mmd_hip.h; one image: 0) under kernel "imq" (WAE's sum of inverse multiquadrics) or
    "rbf" with bandwidth `bandwidth` (None: 2 D, the expected squared distance of two prior draws).  The weight
    alpha + lam - 1 may be any finite value.  `mmd_loss` logs the weighted term.

    Noise: p follows the contract of eps -- drawn on the device after eps, into a buffer of its own, or injected
    (fused_step(..., prior=...)).  An EVALUATION step of this loss also draws p (the five reference losses draw nothing in
    evaluation).  The MMD couples the whole batch: data-parallel steps are not built (fused_step raises under a communicator
    of more than one rank)."""
    KIND = _lib.LOSS_BETAH
    STORED = (('recon_loss', _lib.S_REC), ('kl_loss', _lib.S_KL), ('mmd_loss', None), ('loss', _lib.S_LOSS))

    def __init__(self, alpha=0., lam=1000., kernel="imq", bandwidth=None, **kwargs):
        super().__init__(**kwargs)
        if kernel not in _mmdlib.KERNELS:
            raise ValueError("kernel must be one of {}, got {!r}".format(sorted(_mmdlib.KERNELS), kernel))
        self.alpha, self.lam, self.kernel = float(alpha), float(lam), kernel
        if bandwidth is not None and not float(bandwidth) > 0:
            raise ValueError("bandwidth must be positive, got {!r}".format(bandwidth))
        self.bandwidth = None if bandwidth is None else float(bandwidth)
        self._mmd = {}

    @property
    def beta(self):
        return 1. - self.alpha

    @property
    def weight(self):
        return self.alpha + self.lam - 1.

    def _h(self, D):
        return 2. * D if self.bandwidth is None else self.bandwidth

    def _coefs(self, is_train):
        anneal = linear_annealing(0, 1, self.n_train_steps, self.steps_anneal) if is_train else 1
        return dict(ANNEAL=anneal, BETA=self.beta)

    def _mmd_buf(self, device, name, n):
        """fp64 buffers of the two launches, allocated once: ("ws", B, D) the workspace, ("out",) the value and the three sums."""
        t = self._mmd.get((device,) + name)
        if t is None:
            _lib.note_alloc()
            t = self._mmd[(device,) + name] = torch.zeros(n, dtype=torch.float64, device=device)
        return t

    def _regulariser(self, buf, sc, B, D, is_train, stream, prior=None):
        """w MMD_u on top of the epilogue's rec + anneal * beta * KL in sc.scal[S_LOSS] (dvae_mmd_finish's loss_io: no third
        launch) -> the gradients for the FC chain; evaluation: the value only."""
        if prior is None:
            prior = sc.latent("mmd_prior", B, D)
            record_py(prior.normal_)               # after eps (training), alone in evaluation
        ws = self._mmd_buf(sc.device, ("ws", B, D), _mmdlib.ws_doubles(B, D))
        out = self._mmd_buf(sc.device, ("out",), _mmdlib.OUT_DOUBLES)
        dmu = sc.latent("mmd_dmu", B, D) if is_train else None
        dlv = sc.latent("mmd_dlv", B, D) if is_train else None
        _mmd_launches(buf.z, prior, buf.mu, self.kernel, self._h(D), self.weight, ws, dmu, dlv, out,
                      ptr(sc.scal) + 4 * _lib.S_LOSS, stream)
        return dmu, dlv

    def _replay_key(self, model, data, injected, pol):
        return super()._replay_key(model, data, injected, pol) + (self.kernel, self.bandwidth, self.alpha, self.lam)

    def _store(self, storer, sc, D, keys=None):
        if storer is None:
            return
        vals = sc.scal.tolist()
        mmd = self._mmd[(sc.device, "out")][0].item()           # fp64 [w MMD_u, MMD_u, S_zz, S_pp, S_zp]: a second small copy, on logging steps only
        for key, slot in self.STORED:
            if key == 'kl_loss':
                self._store_kl(storer, vals, D)
            else:
                storer[key].append(mmd if key == 'mmd_loss' else vals[slot])

    def fused_step(self, data, model, optimizer, storer, eps=None, prior=None):
        if self._world()[0] > 1:
            raise NotImplementedError(
                "InfoVAE under data parallelism is not built: the MMD couples the GLOBAL batch, so a sharded step has to gather "
                "the latent samples of every rank first, as the beta-TCVAE estimator does (Comm.all_gather_latents)")
        return super().fused_step(data, model, optimizer, storer, eps=eps, extra_noise=[("mmd_prior_in", prior)])

    def __call__(self, data, recon_data, latent_dist, is_train, storer, latent_sample=None):
        if latent_sample is None:
            if is_train:
                raise ValueError("InfoVaeLoss needs latent_sample in training: the MMD term is a function of the sampled z")
            latent_sample = latent_dist[0]                      # evaluation: the mean
        storer = self._pre_call(is_train, storer)
        sc = self.scratch(recon_data.device)
        rec_loss = _reconstruction_loss(data, recon_data, storer=storer, distribution=self.rec_dist, scratch=sc)
        kl_loss = _kl_normal_loss(*latent_dist, storer, scratch=sc)
        D = latent_sample.shape[1]
        prior = torch.empty_like(latent_sample).normal_()
        mmd_loss = _MmdFn.apply(latent_sample, prior, self.kernel, self._h(D), self.weight)
        anneal_reg = linear_annealing(0, 1, self.n_train_steps, self.steps_anneal) if is_train else 1
        loss = rec_loss + anneal_reg * (self.beta * kl_loss) + mmd_loss
        if storer is not None:
            storer['mmd_loss'].append(mmd_loss.item())
            storer['loss'].append(loss.item())
        return loss


class WeakVaeLoss(_SingleOptimizerLoss):
    """Ada-GVAE / Ada-ML-VAE (Locatello et al. 2020, "Weakly-Supervised Disentanglement Without Compromises";
    disentanglement_lib's weak_vae.py -- the reference has no counterpart) on a batch of image PAIRS: 2 P rows, rows i and P + i
    a pair that shares all but a few factors of variation (data.PairedFactorLoader, or any batch whose halves pair up).

        loss = rec + anneal * beta * KL(q~ || N(0, I)),        both terms means over the 2 P rows

    q~ is the adaptive group posterior (include/dvae_weak_hip.h): per pair and dimension delta = 2 KL(q_a || q_b), the
    threshold tau half way between the pair's largest and smallest delta, and on every dimension with delta < tau both rows
    receive one posterior -- the mean of means and variances (aggregation "gvae") or the product of experts ("mlvae").  The mask
    is a constant for the gradient.  z = m~ + exp(lv~ / 2) eps with eps [2 P, D] under the noise contract of the other losses
    (one normal_, or injected); in evaluation z = m~.  After a step the engine's buf.mu / buf.logvar hold q~.

    The operator sits between mu_logvar_gen and the reparameterisation, inside what the fused FC chain does in one launch:
    the step runs the FC core one launch per layer around it (the path of latent dimensions above 16) and the 4x4 conv ends as
    launches of their own, for every latent dimension.  `shared_dims` logs the mean number of shared dimensions per pair.
    Data-parallel steps are not built (fused_step raises under a communicator of more than one rank)."""
    KIND = _lib.LOSS_BETAH
    STORED = (('recon_loss', _lib.S_REC), ('kl_loss', _lib.S_KL), ('shared_dims', None), ('loss', _lib.S_LOSS))

    def __init__(self, aggregation="gvae", beta=1, **kwargs):
        super().__init__(**kwargs)
        if aggregation not in _weaklib.KINDS:
            raise ValueError("aggregation must be one of {}, got {!r}".format(sorted(_weaklib.KINDS), aggregation))
        self.aggregation = aggregation
        self.beta = beta
        self._weak = {}
        self._shared = None          # the mask of the last step: what `shared_dims` is counted from

    _coefs = BetaHLoss._coefs

    def _begin_step(self, model, data):
        """The step's policy without the fused 4x4 conv ends: there is no chain launch to carry them."""
        pol = super()._begin_step(model, data)._replace(fuse_ends=False)
        model.engine.begin_step(pol)
        return pol

    def _pair_bufs(self, device, P, D):
        """(ml_agg fp32 [2 P, 2 D], shared int64 [P], delta fp32 [P, D]) of the two launches, allocated once per shape."""
        t = self._weak.get((device, P, D))
        if t is None:
            _lib.note_alloc()
            t = self._weak[(device, P, D)] = (torch.empty(2 * P, 2 * D, dtype=torch.float32, device=device),
                                              torch.empty(P, dtype=torch.int64, device=device),
                                              torch.empty(P, D, dtype=torch.float32, device=device))
        return t

    def _replay_key(self, model, data, injected, pol):
        return super()._replay_key(model, data, injected, pol) + (self.aggregation,)

    def _store(self, storer, sc, D, keys=None):
        if storer is None:
            return
        vals = sc.scal.tolist()
        shared = popcount64(self._shared).double().mean().item()     # one more small copy, on logging steps only
        for key, slot in self.STORED:
            if key == 'kl_loss':
                self._store_kl(storer, vals, D)
            else:
                storer[key].append(shared if key == 'shared_dims' else vals[slot])

    def fused_step(self, data, model, optimizer, storer, eps=None):
        _check_pairs(data.shape[0], model.latent_dim)
        if self._world()[0] > 1:
            raise NotImplementedError(
                "Ada-GVAE / Ada-ML-VAE under data parallelism is not built: both members of a pair have to lie on one rank, "
                "which the sharding of a batch by rows does not give")
        # here, not in _device_step: a replayed step does not run that, and `shared_dims` is counted from THIS step's mask
        self._shared = self._pair_bufs(data.device, data.shape[0] // 2, model.latent_dim)[1]
        return super().fused_step(data, model, optimizer, storer, eps=eps)

    def _device_step(self, data, model, sc, eps, is_train):
        """Forward + loss + backward as one stream of launches: the FC core layer by layer around the pair operator."""
        eng = model.engine
        B, D = data.shape[0], model.latent_dim
        buf = eng.buffers(B)
        s = _stream()
        data = eng.input(data, buf)
        if is_train and eps is None:
            eps = sc.latent("eps", B, D)
            record_py(eps.normal_)
        if not is_train:
            eps = None
        op = _PairAggregate(_weaklib.KINDS[self.aggregation], D, *self._pair_bufs(data.device, B // 2, D), s)
        eng.encode_convs(data, buf, chain=False)
        # kl_dim receives the D final values (coef is passed): nothing is left for the epilogue to finish
        eng._fc_layers_fwd(buf, eps, sc.kl_dim, B, B, B, sc.coef, latent_op=op)
        eng.decode_convs(buf, B, fuse_loss=(data, self._rec_code(), sc.coef, sc.partials), ends=False)
        self._finish_loss(sc, 0, D, None, B, None, B, s)
        if not is_train:
            return

        def fc_chain():
            eng._fc_layers_bwd(buf, eps, None, None, None, None, sc.scal, sc.coef, B, latent_op=op)
        self._backward(eng, model, data, buf, B, fc_chain)

    def __call__(self, data, recon_data, latent_dist, is_train, storer, **kwargs):
        raise NotImplementedError(
            "WeakVaeLoss has no loss(data, recon, latent_dist, ...) form: the pairs are aggregated BEFORE z is sampled, so a "
            "reconstruction made from the un-aggregated posterior cannot carry the loss.  Train with fused_step (the native "
            "Trainer does), or build the loss of a model of your own on adaptive_group_posterior(mu, logvar, aggregation)")


class SemiSupervisedVaeLoss(_SingleOptimizerLoss):
    """S2-beta-VAE (Locatello et al. 2020, "Disentangling Factors of Variation Using Few Labels"; disentanglement_lib's
    semi_supervised_vae.py -- the reference has no counterpart): beta-VAE on the whole batch plus a supervised regulariser on
    the few rows of the batch whose factors of variation are known.

        loss = rec + anneal * beta * KL + w_t * R_sup(mu[labelled], labels)

    rec and KL are BetaHLoss's, means over ALL rows of the batch, and steps_anneal acts on the KL term as there.  R_sup runs
    over the labelled rows only and reads the posterior MEANS.  The data set enumerates its factors ``lat_sizes`` by row number
    in row-major order (dSprites, 3D shapes, Cars3D, ...): ``labels`` is int64 [B] on the device, the row number of every image
    of the batch, NEGATIVE for an unlabelled one, and the value index of factor j of row r is (r // stride_j) % size_j -- a
    label tensor never exists.  Factor ``sup_factors[k]`` is tied to latent k, K = len(sup_factors) <= latent_dim and K <= 8;
    the default is every factor with two values or more, in the order of lat_sizes.  With y_ik = value_ik / size_k:

      sup_loss "xent"  sum_i sum_{k<K} BCE-with-logits(mu_ik, y_ik), in the stable form max(x, 0) - x y + log1p(exp(-|x|)); the
                       gradient is sigmoid(mu_ik) - y_ik;
      sup_loss "l2"    sum_i sum_{k<K} (mu_ik - y_ik)^2;
      sup_loss "cov"   sum_{(d, k), d != k} C_dk^2 with C [D, K] the biased cross-covariance of mu and the factor value INDICES
                       (not normalised, as in disentanglement_lib) over the labelled rows; the entries d = k are left out; the
                       gradient is (2 / n_lab) sum_{k != d} C_dk (v_ik - mean v_k), so every one of the D latents receives one.

    sup_reduction "sum" (disentanglement_lib's default) or "mean": xent and l2 divided by the number of labelled rows, on the
    device (cov is a function of means already and is the same under both).  w_t is gamma_sup (sup_anneal "fixed"), or
    linear_annealing(0, gamma_sup, step, sup_anneal_steps) in training (sup_anneal "anneal"; evaluation: gamma_sup); the kernels
    read it from the step's staged coefficient buffer, so a replayed plan or hipGraph sees this step's value.  With no labelled
    row in the batch R_sup = 0 and every gradient of it is an exact zero; with ``labels=None`` the two launches are skipped
    and the step is BetaHLoss's.  `sup_loss` logs R_sup (after the reduction, without w_t), `n_labelled` the labelled rows.

    NOT built: disentanglement_lib's "embed" regulariser, the learnt scale of its l2 form, its "fine_tune" annealer, S2 on top
    of the FactorVAE / beta-TCVAE / DIP terms, and binned or noisy labels (labels are the exact factor values).  The labelled
    rows couple the batch: data-parallel steps are not built (fused_step raises under a communicator of more than one rank)."""
    KIND = _lib.LOSS_BETAH
    STORED = (('recon_loss', _lib.S_REC), ('kl_loss', _lib.S_KL), ('sup_loss', None), ('n_labelled', None), ('loss', _lib.S_LOSS))
    takes_labels = True           # Trainer / Evaluator pass the second item of a batch as fused_step(..., labels=)

    def __init__(self, lat_sizes, sup_loss="xent", gamma_sup=1., beta=4, sup_reduction="sum", sup_anneal="fixed",
                 sup_anneal_steps=0, sup_factors=None, latent_dim=None, n_data=None, **kwargs):
        super().__init__(**kwargs)
        if sup_loss not in _semilib.KINDS:
            raise ValueError("sup_loss must be one of {}, got {!r}".format(sorted(_semilib.KINDS), sup_loss))
        if sup_reduction not in _semilib.REDUCTIONS:
            raise ValueError("sup_reduction must be one of {}, got {!r}".format(sorted(_semilib.REDUCTIONS), sup_reduction))
        if sup_anneal not in ("fixed", "anneal"):
            raise ValueError("sup_anneal must be 'fixed' or 'anneal', got {!r}".format(sup_anneal))
        self.lat_sizes = tuple(int(s) for s in lat_sizes)
        if not self.lat_sizes or min(self.lat_sizes) < 1:
            raise ValueError("lat_sizes must be positive factor sizes, got {!r}".format(lat_sizes))
        n_rows = 1
        for s in self.lat_sizes:
            n_rows *= s
        if n_data is not None and n_rows != int(n_data):
            raise ValueError("lat_sizes {} enumerate {} images, the data set has {}".format(self.lat_sizes, n_rows, int(n_data)))
        if sup_factors is None:
            sup_factors = [j for j, s in enumerate(self.lat_sizes) if s >= 2]
        self.factors = tuple(int(j) for j in sup_factors)
        if not self.factors or len(set(self.factors)) != len(self.factors) or \
                not all(0 <= j < len(self.lat_sizes) for j in self.factors):
            raise ValueError("sup_factors must be distinct indices into lat_sizes {} (at least one), got {!r}".format(
                self.lat_sizes, sup_factors))
        if len(self.factors) > _semilib.MAX_K:
            raise ValueError("at most {} supervised factors, got {}".format(_semilib.MAX_K, len(self.factors)))
        self.sup_loss, self.sup_reduction, self.sup_anneal = sup_loss, sup_reduction, sup_anneal
        self.gamma_sup, self.sup_anneal_steps, self.beta = float(gamma_sup), int(sup_anneal_steps), beta
        self._table = _semilib.factor_table(self.lat_sizes, self.factors)      # host arrays: recorded launches hold their addresses
        self._semi = {}
        self._labelled_now = False     # whether the step under way has a rows tensor: its launches exist, `out` is this step's
        if latent_dim is not None:
            self._check_dims(1, int(latent_dim))

    @property
    def n_factors(self):
        return len(self.factors)

    def _check_dims(self, rows, D):
        """What a batch has to satisfy, before any device work."""
        if self.n_factors > D:
            raise ValueError("{} supervised factors need latent_dim >= {} (factor k is tied to latent k), got {}".format(
                self.n_factors, self.n_factors, D))
        if D > _semilib.MAX_D:
            raise ValueError("the semi-supervised loss takes latent_dim <= {}, got {}".format(_semilib.MAX_D, D))
        if not 1 <= rows <= _semilib.MAX_ROWS:
            raise ValueError("the semi-supervised loss takes batches of 1 to {} rows, got {}".format(_semilib.MAX_ROWS, rows))

    @staticmethod
    def _check_labels(labels, rows, device):
        if not (torch.is_tensor(labels) and labels.dtype == torch.int64 and tuple(labels.shape) == (rows,)):
            raise ValueError("labels must be an int64 tensor of {} row numbers (negative: unlabelled), got {!r}".format(
                rows, (getattr(labels, "dtype", None), tuple(getattr(labels, "shape", ()))) if torch.is_tensor(labels) else labels))
        if labels.device != device:
            raise ValueError("labels must lie on the batch's device {}, got {}".format(device, labels.device))

    def sup_weight(self, is_train):
        """w_t of the step under way."""
        if self.sup_anneal == "fixed" or not is_train:
            return self.gamma_sup
        return linear_annealing(0, self.gamma_sup, self.n_train_steps, self.sup_anneal_steps)

    def _coefs(self, is_train):
        # w_t rides in the GAMMA slot of the staged coefficients: the BETAH epilogue and FC chain do not read it (loss.hip:
        # loss_finalize_body; latent_math.h: load_tc_coef is the beta-TCVAE estimator's)
        anneal = linear_annealing(0, 1, self.n_train_steps, self.steps_anneal) if is_train else 1
        return dict(ANNEAL=anneal, BETA=self.beta, GAMMA=self.sup_weight(is_train))

    def _semi_buf(self, device, name, n):
        """fp64 buffers of the two launches, allocated once: ("ws", B, D) the workspace, ("out", D) value, count and C."""
        t = self._semi.get((device,) + name)
        if t is None:
            _lib.note_alloc()
            t = self._semi[(device,) + name] = torch.zeros(n, dtype=torch.float64, device=device)
        return t

    def _regulariser(self, buf, sc, B, D, is_train, stream, rows=None):
        """w_t R_sup on top of the epilogue's rec + anneal * beta * KL in sc.scal[S_LOSS] (dvae_semi_grad's loss_io: no third
        launch) -> the gradient for the FC chain; evaluation: the value only; no rows: nothing."""
        if rows is None:
            return None
        K = self.n_factors
        ws = self._semi_buf(sc.device, ("ws", B, D), _semilib.ws_doubles(B, D, K))
        out = self._semi_buf(sc.device, ("out", D), _semilib.out_doubles(D, K))
        dmu = sc.latent("semi_dmu", B, D) if is_train else None
        _semi_launches(buf.mu, rows, K, self._table, _semilib.KINDS[self.sup_loss], _semilib.REDUCTIONS[self.sup_reduction],
                       ptr(sc.coef) + 4 * _lib.C_GAMMA, ws, dmu, out, ptr(sc.scal) + 4 * _lib.S_LOSS, stream)
        return dmu, None

    def _replay_key(self, model, data, injected, pol):
        return super()._replay_key(model, data, injected, pol) + (
            self.sup_loss, self.sup_reduction, self.sup_anneal, self.sup_anneal_steps, self.gamma_sup, self.lat_sizes,
            self.factors, self._labelled_now)

    def _store(self, storer, sc, D, keys=None):
        if storer is None:
            return
        vals = sc.scal.tolist()
        sup, n_lab = 0.0, 0.0
        if self._labelled_now:
            sup, n_lab = self._semi[(sc.device, "out", D)][:2].tolist()     # fp64 [R, n_lab, C]: a second small copy, on logging steps only
        for key, slot in self.STORED:
            if key == 'kl_loss':
                self._store_kl(storer, vals, D)
            else:
                storer[key].append({'sup_loss': sup, 'n_labelled': n_lab}[key] if slot is None else vals[slot])

    def fused_step(self, data, model, optimizer, storer, eps=None, labels=None):
        """labels: int64 [B] on the batch's device (row numbers, negative: unlabelled), or None: all unlabelled, and the
        regulariser's launches are skipped.  The rows go through _run_step's static buffers as eps does: a recorded plan reads
        them from a buffer that is refreshed every step."""
        if self._world()[0] > 1:
            raise NotImplementedError(
                "S2-VAE under data parallelism is not built: the labelled rows of the GLOBAL batch share one count (and, for "
                "cov, one covariance), so a sharded step has to gather the means and rows of every rank first")
        self._check_dims(data.shape[0], model.latent_dim)
        if labels is not None:
            self._check_labels(labels, data.shape[0], data.device)
        self._labelled_now = labels is not None
        return super().fused_step(data, model, optimizer, storer, eps=eps, extra_noise=[("s2_rows", labels)])

    def __call__(self, data, recon_data, latent_dist, is_train, storer, labels=None, **kwargs):
        storer = self._pre_call(is_train, storer)
        sc = self.scratch(recon_data.device)
        rec_loss = _reconstruction_loss(data, recon_data, storer=storer, distribution=self.rec_dist, scratch=sc)
        kl_loss = _kl_normal_loss(*latent_dist, storer, scratch=sc)
        mu = latent_dist[0]
        self._check_dims(mu.shape[0], mu.shape[1])
        anneal_reg = linear_annealing(0, 1, self.n_train_steps, self.steps_anneal) if is_train else 1
        loss = rec_loss + anneal_reg * (self.beta * kl_loss)
        sup_loss = None
        if labels is not None:
            self._check_labels(labels, mu.shape[0], mu.device)
            sup_loss = _SemiFn.apply(mu, labels, self.n_factors, self._table, _semilib.KINDS[self.sup_loss],
                                     _semilib.REDUCTIONS[self.sup_reduction])
            loss = loss + self.sup_weight(is_train) * sup_loss
        if storer is not None:
            storer['sup_loss'].append(0.0 if sup_loss is None else sup_loss.item())
            storer['n_labelled'].append(0.0 if labels is None else float((labels >= 0).sum().item()))
            storer['loss'].append(loss.item())
        return loss


class BetaBLoss(_SingleOptimizerLoss):
    """losses.py:156-202."""
    KIND = _lib.LOSS_BETAB

    def __init__(self, C_init=0., C_fin=20., gamma=100., **kwargs):
        super().__init__(**kwargs)
        self.gamma = gamma
        self.C_init = C_init
        self.C_fin = C_fin

    def _capacity(self, is_train):
        return (linear_annealing(self.C_init, self.C_fin, self.n_train_steps, self.steps_anneal)
                if is_train else self.C_fin)

    def _coefs(self, is_train):
        return dict(ANNEAL=1.0, BETA=self.gamma, CAP=self._capacity(is_train))

    def __call__(self, data, recon_data, latent_dist, is_train, storer, **kwargs):
        storer = self._pre_call(is_train, storer)
        sc = self.scratch(recon_data.device)
        rec_loss = _reconstruction_loss(data, recon_data, storer=storer, distribution=self.rec_dist, scratch=sc)
        kl_loss = _kl_normal_loss(*latent_dist, storer, scratch=sc)
        C = self._capacity(is_train)
        loss = rec_loss + self.gamma * (kl_loss - C).abs()
        if storer is not None:
            storer['loss'].append(loss.item())
        return loss


class BtcvaeLoss(_SingleOptimizerLoss):
    """losses.py:316-391 (is_mss=True default, never overridden by get_loss_f)."""
    KIND = _lib.LOSS_BTCVAE
    STORED = (('recon_loss', _lib.S_REC), ('loss', _lib.S_LOSS), ('mi_loss', _lib.S_MI), ('tc_loss', _lib.S_TC),
              ('dw_kl_loss', _lib.S_DWKL), ('kl_loss', _lib.S_KL))

    def __init__(self, n_data, alpha=1., beta=6., gamma=1., is_mss=True, **kwargs):
        super().__init__(**kwargs)
        self.n_data = n_data
        self.beta = beta
        self.alpha = alpha
        self.gamma = gamma
        self.is_mss = is_mss

    def _coefs(self, is_train):
        anneal = linear_annealing(0, 1, self.n_train_steps, self.steps_anneal) if is_train else 1
        return dict(ANNEAL=anneal, ALPHA=self.alpha, BETA=self.beta, GAMMA=self.gamma)

    def _estimator(self, eng, buf, sc, B, D, is_train):
        """The B x B estimator, forward AND backward (it needs z, mu, logvar and the coefficients only), on the side stream --
        sharded: the exchange stream -- beside the decoder forward -> (rowstats, dz, dmu, dlogvar, xbuf); xbuf: the buffer a
        sharded step's late epilogue sums over the ranks (else None)."""
        world = self._world()[0]
        ew, er = self._est_world()            # the estimator's view of the sharding (local mode: one shard = one batch)
        Be = B * ew
        dz_x = dmu_x = dlv_x = xbuf = None
        with torch.cuda.stream(eng.aux_stream if world > 1 else eng.side_stream):
            ss = _stream()
            zg, mug, lvg = buf.z, buf.mu, buf.logvar
            if ew > 1:
                zg, mug, lvg = self.comm.all_gather_latents(buf.z, buf.mu, buf.logvar)
            rowstats = sc.latent("rowstats", B, _lib.rowstats_stride(D))
            tc_tmp = sc.latent("tc_tmp", 1, _lib.btcvae_tmp_floats(Be, B, D))
            call("dvae_btcvae_fwd", ptr(zg), ptr(mug), ptr(lvg), Be, D, er * B, B, int(self.is_mss), ptr(sc.log_w),
                 ptr(tc_tmp), ptr(rowstats), ss)
            if is_train:
                dz_x = sc.latent("dz_tc", B, D)
                # (dmu, dlogvar) of ALL columns: two slabs of one buffer, followed by the packed loss sums -- sharded, the
                # lot is summed over the ranks by ONE all-reduce in the step's late epilogue (Comm.all_reduce_cols_sums)
                slabs = sc.latent("xbuf", 1, 2 * Be * D + _lib.npack(D)).view(-1)
                dmu_x, dlv_x = slabs[:Be * D].view(Be, D), slabs[Be * D:2 * Be * D].view(Be, D)
                call("dvae_btcvae_bwd", ptr(zg), ptr(mug), ptr(lvg), ptr(rowstats), Be, D, er * B, B,
                     int(self.is_mss), ptr(sc.log_w), ptr(sc.coef), ptr(tc_tmp), ptr(dz_x), ptr(dmu_x), ptr(dlv_x), ss)
                if ew > 1:
                    xbuf = slabs
                    dmu_x, dlv_x = dmu_x[er * B:(er + 1) * B], dlv_x[er * B:(er + 1) * B]
                if world > ew:                # local estimator: its mean runs over B, the loss over B * world
                    for t_ in (dz_x, dmu_x, dlv_x):
                        scale_(t_, 1.0 / world)
        return rowstats, dz_x, dmu_x, dlv_x, xbuf

    def __call__(self, data, recon_batch, latent_dist, is_train, storer, latent_sample=None):
        storer = self._pre_call(is_train, storer)
        sc = self.scratch(recon_batch.device)
        rec_loss = _reconstruction_loss(data, recon_batch, storer=storer, distribution=self.rec_dist, scratch=sc)
        terms = _BtcvaeFn.apply(latent_sample, latent_dist[0], latent_dist[1], self.n_data, self.is_mss, sc)
        mi_loss, tc_loss, dw_kl_loss = terms[0], terms[1], terms[2]
        anneal_reg = linear_annealing(0, 1, self.n_train_steps, self.steps_anneal) if is_train else 1
        loss = rec_loss + (self.alpha * mi_loss + self.beta * tc_loss + anneal_reg * self.gamma * dw_kl_loss)
        if storer is not None:
            storer['loss'].append(loss.item())
            storer['mi_loss'].append(mi_loss.item())
            storer['tc_loss'].append(tc_loss.item())
            storer['dw_kl_loss'].append(dw_kl_loss.item())
            with torch.no_grad():
                _ = _kl_normal_loss(latent_dist[0].detach(), latent_dist[1].detach(), storer, scratch=sc)
        return loss


class FactorKLoss(BaseLoss):
    """losses.py:205-313.  ``call_optimize`` runs the whole two-optimizer iteration on the HIP
    kernels, including quirk Q1 (the encoder also receives d[0.5 CE(D(z1),0)]/dz1 because the
    reference does not detach d_z and steps the VAE optimizer after d_tc_loss.backward())."""

    KIND = _lib.LOSS_FACTOR
    STORED = (('recon_loss', _lib.S_REC), ('kl_loss', _lib.S_KL), ('loss', _lib.S_LOSS), ('tc_loss', _lib.S_TC),
              ('discrim_loss', _lib.S_DTC))

    def __init__(self, device, gamma=10., disc_kwargs={}, optim_kwargs=dict(lr=5e-5, betas=(0.5, 0.9)), **kwargs):
        super().__init__(**kwargs)
        self.gamma = gamma
        self.device = device
        self.discriminator = Discriminator(**disc_kwargs).to(self.device)
        optim_kwargs = dict(optim_kwargs)
        if torch.device(self.device).type == "cuda":
            optim_kwargs.setdefault("fused", True)   # same Adam arithmetic, one multi-tensor kernel
        self.optimizer_d = torch.optim.Adam(self.discriminator.parameters(), **optim_kwargs)

    def __call__(self, *args, **kwargs):
        raise ValueError("Use `call_optimize` to also train the discriminator")  # losses.py:240-241

    _PERM_RING = 4

    def _draw_perms(self, D, n):
        """D independent torch.randperm(n) draws (losses.py:505, CPU generator, the reference's order) into the next slot of
        a small ring of pinned [D, n] int64 buffers -> (buffer, slot); slot[1] is the event that marks the slot's last
        host-to-device copy (waited for before the slot is overwritten: normally long past)."""
        ring = self.__dict__.setdefault("_perm_ring", {})
        ent = ring.get((D, n))
        if ent is None:
            ent = ring[(D, n)] = {"slots": [[torch.empty(D, n, dtype=torch.int64).pin_memory(), None]
                                            for _ in range(self._PERM_RING)], "next": 0}
        slot = ent["slots"][ent["next"]]
        ent["next"] = (ent["next"] + 1) % self._PERM_RING
        if slot[1] is not None:
            slot[1].synchronize()
        for d in range(D):
            torch.randperm(n, out=slot[0][d])
        return slot[0], slot

    def _device_step(self, data, model, sc, eps1, eps2, perms):
        """Training iteration of FactorVAE as one stream of launches (no host-dependent values):
        VAE forward on both halves, discriminator on (z1, z_perm), both backward passes."""
        eng = model.engine
        disc = self.discriminator
        D = model.latent_dim
        Bh = data.size(0) // 2
        world = self._world()[0]
        s = _stream()
        # the N(0,1) draws of both halves in ONE [2*Bh, D] buffer (rows < Bh: data1, losses.py:254; the rest:
        # sample_latent(data2), losses.py:286) -- two separate draws, like the reference, into its two halves
        eps12 = sc.latent("eps12", 2 * Bh, D)
        if eps1 is None:
            record_py(eps12[:Bh].normal_)
            record_py(eps12[Bh:].normal_)
        else:
            record_py(eps12[:Bh].copy_, eps1)
            record_py(eps12[Bh:].copy_, eps2)
        buf = eng.buffers(data.size(0))
        data = eng.input(data, buf)
        ends = eng.encode_convs(data, buf, n=2 * Bh, chain=True)                  # data1 and data2 in one pass
        # FC core of both halves in one launch; KL only over data1 with the half batch as denominator (losses.py:255-259),
        # decoder only for data1
        eng.fc_chain_fwd(buf, eps12, sc.kl_dim, 2 * Bh, n_kl=Bh, n_dec=Bh, coef=sc.coef, ends=ends)
        klb = eng.kl_blocks(2 * Bh)
        eng.decode_convs(buf, Bh, fuse_loss=(data, self._rec_code(), sc.coef, sc.partials), ends=ends)
        # z_perm: permute across the (global) half batch, losses.py:287
        zin = sc.latent("disc_in", 2 * Bh, D)
        copy_flat_(zin[:Bh], buf.z[:Bh])
        z2 = buf.z[Bh:2 * Bh]
        ew, er = self._est_world()                # scope of permute_dims: global half batch, or this shard ("local")
        z2g = self.comm.all_gather_rows(z2) if ew > 1 else z2
        zperm_g = sc.latent("zperm_g", Bh * ew, D)
        call("dvae_permute_dims", ptr(z2g.contiguous()), ptr(perms), ptr(zperm_g), Bh * ew, D, s)
        copy_flat_(zin[Bh:], zperm_g[er * Bh:(er + 1) * Bh])
        logits = disc.forward_raw(zin, 2 * Bh)                        # D(z1) and D(z_perm) in one pass
        g_dtc = sc.latent("g_dtc", 2 * Bh, 2)
        g_tc = sc.latent("g_tc", Bh, 2)
        call("dvae_disc_losses", ptr(logits), Bh, ptr(sc.coef), ptr(sc.disc_sums), ptr(g_dtc), ptr(g_tc), s)
        if world > 1:
            # the CE / tc means run over the global half batch
            scale_(g_dtc, 1.0 / world)
            scale_(g_tc, 1.0 / world)
        # the scalar epilogue (13 us; sharded: KL finish + pack + all-reduce of the packed sums + finalize) is first needed by
        # the FC chain's input gradients, after the discriminator's and the decoder's backward passes: deferred (_defer_loss)
        wait = None
        if eng.policy.late_join:
            wait = self._defer_loss(eng, lambda stream, on: self._finish_loss(sc, klb, D, None, 0, sc.disc_sums, Bh * world,
                                                                              stream, on))
        else:
            self._finish_loss(sc, klb, D, None, 0, sc.disc_sums, Bh * world, s)
        # discriminator backward of d_tc_loss (weight grads + dz), losses.py:303-304
        # (its six weight gradients: on the side stream, behind one fork after the input-gradient chain)
        side_wg = eng.policy.disc_wgrad_side
        # the second chain of input gradients (the tc term of vae_loss through D: first half, no weight gradients) depends on
        # nothing the first one computes and could run beside it on the engine's third stream.  Measured, NOT shipped (A/B under
        # DVAE_DEBUG=1, same box: factor_dsprites 0.583 vs 0.579-0.585 ms, factor_celeba 1.905 vs 1.885-1.892, tensor 512
        # 0.831 vs 0.788-0.819: profiles/r05_v35_disc_chain2_ab.txt): the fork and the join cost the critical path what the
        # overlap of two launch-bound chains buys, and at 2048 rows both chains fill the chip anyway.
        par2 = eng.policy.disc_chain2_aux
        dz_b = None
        if par2:
            call("dvae_stream_order", s, eng._aux_raw())
            dz_b = disc.backward_raw(zin, g_tc, 2 * Bh, rows=Bh, wgrad=False, chain="g2", stream=eng._aux_raw(), ws="aux")
        dz_a = disc.backward_raw(zin, g_dtc, 2 * Bh, wgrad=True, chain="g", side=eng if side_wg else None)
        pending = []
        if world > 1:      # the 16 MB discriminator gradients are final: their all-reduce runs under the whole VAE backward
            with torch.cuda.stream(eng.side_stream if side_wg else torch.cuda.current_stream()):
                pending.append(self.comm.all_reduce_async(disc.arena.grad))
        # tc term of vae_loss through D: dgrad only, first half (its disc weight grads are zeroed at :303)
        if dz_b is None:
            dz_b = disc.backward_raw(zin, g_tc, 2 * Bh, rows=Bh, wgrad=False, chain="g2")

        def fc_chain():
            # dz_a: quirk Q1 (the encoder also receives d[0.5 CE(D(z1),0)]/dz1); dz_b: the tc term through D
            if par2:
                call("dvae_stream_order", eng._aux_raw(), s)
            if wait is not None:
                wait()
            eng.fc_chain_bwd(buf, eps12[:Bh], dz_a, dz_b, None, None, sc.scal, sc.coef, Bh)
        self._backward(eng, model, data, buf, Bh, fc_chain, pending)

    def _eval_step(self, data, model, sc):
        """Evaluation: vae_loss only (losses.py:276-278) on data1, z = mean; the discriminator on z1."""
        eng, disc = model.engine, self.discriminator
        D = model.latent_dim
        Bh = data.size(0) // 2
        s = _stream()
        buf = eng.buffers(data.size(0))
        data = eng.input(data, buf)
        ends = eng.encode_convs(data, buf, n=Bh, chain=True)
        # KL over data1 with the half batch as denominator (losses.py:255-259)
        eng.fc_chain_fwd(buf, None, sc.kl_dim, Bh, coef=sc.coef, ends=ends)
        if eng.kl_blocks(Bh):
            call("dvae_kl_finish", ptr(sc.kl_dim), eng.kl_blocks(Bh), ptr(sc.coef), D, s)
        eng.decode_convs(buf, Bh, fuse_loss=(data, self._rec_code(), sc.coef, sc.partials), ends=ends)
        logits = disc.forward_raw(buf.z, Bh)
        g_dtc = sc.latent("g_dtc", 2 * Bh, 2)
        lg2 = sc.latent("lg2", 2 * Bh, 2)
        lg2[:Bh].copy_(logits[:Bh]); lg2[Bh:].copy_(logits[:Bh])
        call("dvae_disc_losses", ptr(lg2), Bh, ptr(sc.coef), ptr(sc.disc_sums), ptr(g_dtc), None, s)
        call("dvae_loss_pack", ptr(sc.partials), ptr(sc.kl_dim), D, None, 0, ptr(sc.disc_sums), ptr(sc.packed), s)
        if self._world()[0] > 1:
            self.comm.all_reduce(sc.packed)
        call("dvae_loss_finalize", self.KIND, ptr(sc.packed), D, Bh * self._world()[0], ptr(sc.coef), ptr(sc.scal), s)

    def call_optimize(self, data, model, optimizer, storer, noise=None):
        """noise: optional (eps1[Bh,D], eps2[Bh,D], perms int64[D,Bh]) injected for parity;
        by default eps are drawn on the device and the permutations with torch.randperm on the
        CPU generator, in the reference's order (losses.py:254,286,505)."""
        is_train = model.training
        storer = self._pre_call(is_train, storer)
        D = model.latent_dim
        Bh = data.size(0) // 2
        sc = self.scratch(data.device).for_latent_dim(D)
        anneal = linear_annealing(0, 1, self.n_train_steps, self.steps_anneal) if is_train else 1
        sc.set_coef_host(INV_B=1.0 / (Bh * self._world()[0]), ANNEAL=anneal, BETA=self.gamma)
        model.engine.stage(sc.coef, sc.coef_host)       # ONE launch: this step's weight images + its loss coefficients
        data = data.contiguous()
        pol = self._begin_step(model, data)
        if not is_train:
            self._eval_step(data, model, sc)
            self._store(storer, sc, D, self.STORED[:-1])
            return sc.scal[_lib.S_LOSS]
        eps1, eps2, perms = noise if noise is not None else (None, None, None)     # (eps: drawn on the device in _device_step)
        slot = None
        if perms is None:
            # CPU generator (shared seed across ranks), reference order losses.py:505 -- drawn straight into a pinned
            # staging buffer: the copy to the device is then truly asynchronous (from pageable memory it blocks the host
            # until every launch enqueued before it has run, i.e. the host could never run ahead of the GPU)
            perms, slot = self._draw_perms(D, Bh * self._est_world()[0])
        perms = self._static_buf("perms", perms.to(dtype=torch.int64))      # device copy (non-blocking from the pinned ring)
        if slot is not None:
            slot[1] = torch.cuda.Event()
            slot[1].record()                          # the staging buffer is free again once this has passed
        self._run_step(model, data, pol, [("eps1", eps1), ("eps2", eps2)], noise is not None, (self.discriminator.arena.flat.data_ptr(),),
                       lambda data, eps1, eps2: self._device_step(data, model, sc, eps1, eps2, perms))
        model.assign_grads()
        self.discriminator.assign_grads()
        optim.step(optimizer)         # optimizer.step(), losses.py:307
        optim.step(self.optimizer_d)  # losses.py:308
        self._store(storer, sc, D)
        return sc.scal[_lib.S_LOSS]
