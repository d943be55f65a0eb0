"""-m gpu: the separability library (libdvae_sep_hip.so, csrc/latent_loo.hip; Evaluator.compute_separability_scores) against the
fp64 restatement of tests/sep_ref.py.

The switches of the launcher, and the case on each side of each:
  * the kernel: D <= 16 runs k_loo_lse<DP> with DP = D rounded up to an even number -- DP 2 (D 1 with a padding dimension, D 2
    without), 4 (D 4), 6 (D 5, padded), 8 (D 7), 10 (D 10), 12 (D 12), 14 (D 13), 16 (D 15 padded, D 16); D >= 17 runs the
    run-time-D kernel k_loo_lse_wide (D 17, 31, MAX_D);
  * gridDim.z of the run-time-D kernel, groups of GROUP = 16 of the D + 1 rows: D 17 -> 2 groups, the second holding row 16 and
    the joint row; D 31 -> 2 full groups, the joint row the last of the second; MAX_D = 64 -> 5 groups, the last holding the joint
    row alone;
  * chunks of the data set (gridDim.y): N = 7, CHUNK -> one chunk (N = 7: one padding record); CHUNK + 1 -> two chunks, both
    ending in padding records; 2 CHUNK + 1 -> three;
  * the cap of the chunk count by the sample blocks: S = 262400 (1025 blocks) with N = CHUNK + 1 -> one chunk where fewer samples
    get two (test_chunk_cap_by_sample_blocks);
  * sample blocks (gridDim.x): S = 1, 256 -> one (S = 1: 255 idle threads); 257 -> a second, ragged one.

Tolerance per sample: err <= B (2e-6 |ref| + 2e-6).  On the grid tables B = 1 (tests/test_sep_host.py shows that fp32 arithmetic
that ADDS the other terms stays inside it, and that T - t_i would miss it by three orders of magnitude and more).  On every other
table, for row i, B = max(1, 2 b_i) where b_i is the multiple of the same tolerance that the shipped dvae_eval_joint_logq reaches
here on the table with column i deleted (row D: the full table); the factor 2 covers the different (prefix + suffix) order of the
same D - 1 fp32 additions.  H (fp64) is held to the same bound applied to the mean.  Every multiple is printed.
dvae_sep_cond_terms: |err| <= 8 S 2^-53 mean|term| (the fp64 accumulation, which is all the kernel rounds: it widens its fp32
inputs exactly) + 1e-6 |ref| (what the issue of this feature grants for the rounding of fp32 inputs; unused by this kernel)."""
import functools
import json
import logging
import math

import numpy as np
import pytest
import torch

import decomp_ref
import sep_ref as R
from gpu_util import DEV, stream
from guard_util import Guarded, run_contract
from disvae_amd import _evallib, _seplib, Evaluator

pytestmark = pytest.mark.gpu
L = _seplib.CHUNK
MAX_D = _seplib.MAX_D
FAMILIES = {"broad": (-2.0, 0.5), "sharp": (-10.0, 1.0)}
SHAPES = [(7, 1, 1), (7, 4, 257), (L, 5, 256), (L + 1, 10, 257), (2 * L + 1, 4, 257), (L + 1, 16, 256), (7, 17, 257), (L + 1, 17, 1),
          (2 * L + 1, 1, 256), (64, MAX_D, 33), (L, 10, 1)]
# the widths and group counts the shapes above do not reach: about the path, the broad family only
PATH_SHAPES = [(300, 2, 70), (300, 7, 70), (300, 12, 70), (300, 13, 70), (300, 15, 70), (40, 31, 9)]
CASES = [(N, D, S, f) for f in sorted(FAMILIES) for N, D, S in SHAPES] + [(N, D, S, "broad") for N, D, S in PATH_SHAPES] + \
    [(int(np.prod(g)), len(g), 64, "grid") for g in R.GRIDS]
GRID_OF = {(int(np.prod(g)), len(g)): g for g in R.GRIDS}


@functools.lru_cache(maxsize=None)
def problem(N, D, S, family):
    """Inputs (fp32 numpy) and their fp64 [D + 1, S] log-densities: computed once, shared by the tests, never modified."""
    if family == "grid":
        mean, logvar, rows, eps = R.grid_table(GRID_OF[(N, D)], S, seed=1)
    else:
        mean, logvar, rows, eps = (t.numpy() for t in decomp_ref.clustered_posteriors(N, D, S, seed=1000 * D + N % 997,
                                                                                      logvar_range=FAMILIES[family]))
    z = R.sample_z(mean, logvar, rows, eps)
    assert z.shape == eps.shape == (S, D) and mean.shape == logvar.shape == (N, D) and rows.shape == (S,)
    ref = R.loo_logq(z, mean, logvar)
    return mean, logvar, rows, eps, z, ref


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype).contiguous()


def run_loo(mean, logvar, z, st=None, ws_fill=float("nan")):
    """dvae_sep_loo_logq on a poisoned workspace -> (logq [D + 1, S], H [D + 1]) as fp64 numpy (H as the kernel's fp64)."""
    (N, D), S = mean.shape, z.shape[0]
    assert z.shape == (S, D) and logvar.shape == (N, D)                      # the kernels trust these sizes
    need = _seplib.lib().dvae_sep_loo_logq_ws_floats(N, D, S)
    assert need > 0
    zd, md, ld = _dev(z), _dev(mean), _dev(logvar)
    ws = torch.full((need,), ws_fill, device=DEV)
    logq = torch.full((D + 1, S), float("nan"), device=DEV)
    H = torch.full((D + 1,), float("nan"), dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    _seplib.call("dvae_sep_loo_logq", zd.data_ptr(), md.data_ptr(), ld.data_ptr(), N, D, S, ws.data_ptr(), logq.data_ptr(),
                 H.data_ptr(), stream() if st is None else st)
    torch.cuda.synchronize()
    return logq.cpu().double().numpy(), H.cpu().numpy()


def run_joint(mean, logvar, z):
    """The shipped dvae_eval_joint_logq -> logqz [S] as fp64 numpy."""
    (N, D), S = mean.shape, z.shape[0]
    zd, md, ld = _dev(z), _dev(mean), _dev(logvar)
    ws = torch.full((_evallib.lib().dvae_eval_joint_logq_ws_floats(N, D, S),), float("nan"), device=DEV)
    logqz, H = torch.empty(S, device=DEV), torch.empty(1, device=DEV)
    _evallib.call("dvae_eval_joint_logq", zd.data_ptr(), md.data_ptr(), ld.data_ptr(), N, D, S, ws.data_ptr(), logqz.data_ptr(),
                  H.data_ptr(), stream())
    torch.cuda.synchronize()
    return logqz.cpu().double().numpy()


def bounds(mean, logvar, z, ref, family):
    """B of every row of the [D + 1, S] result (see the module docstring), and the shipped kernel's multiples b."""
    D = mean.shape[1]
    if family == "grid":
        return [1.0] * (D + 1), [None] * (D + 1)
    b = []
    for i in range(D + 1):
        cols = [d for d in range(D) if d != i]
        if not cols:
            b.append(0.0)                                                     # D = 1, row 0: the empty sum, no table to run
        else:
            b.append(R.tolerance_multiple(run_joint(mean[:, cols], logvar[:, cols], z[:, cols]), ref[i]))
    return [max(1.0, 2.0 * v) for v in b], b


# ---- 1. parity of logq [D + 1, S] and H -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,S,family", CASES)
def test_logq_vs_fp64(N, D, S, family):
    mean, logvar, rows, eps, z, ref = problem(N, D, S, family)
    assert np.isfinite(ref).all()
    got, H = run_loo(mean, logvar, z)
    B, b = bounds(mean, logvar, z, ref, family)
    what = "N%d D%d S%d %s" % (N, D, S, family)
    assert got.shape == (D + 1, S) and np.isfinite(got).all() and np.isfinite(H).all(), what
    mult = [R.tolerance_multiple(got[i], ref[i]) for i in range(D + 1)]
    Href = -ref.mean(axis=1)
    multH = [abs(H[i] - Href[i]) / (2e-6 * abs(Href[i]) + 2e-6) for i in range(D + 1)]
    worst = int(np.argmax([m / B[i] for i, m in enumerate(mult)]))
    print("%s: worst row %d: err / tol %.3f (B %.3f, shipped kernel %s); max over rows %.3f; H: max err / tol %.3g"
          % (what, worst, mult[worst], B[worst], b[worst], max(mult), max(multH)))
    for i in range(D + 1):
        assert mult[i] <= B[i], (what, "row", i, mult[i], B[i], b[i])
        assert multH[i] <= B[i], (what, "H", i, multH[i], B[i])
    # row D is the joint log-density: the shipped kernel on the same inputs, at the same per-sample tolerance
    joint = run_joint(mean, logvar, z)
    against = float((np.abs(got[D] - joint) / (2e-6 * np.abs(ref[D]) + 2e-6)).max())
    print("%s: row D against dvae_eval_joint_logq: %.3f x tolerance (B %.3f)" % (what, against, B[D]))
    assert against <= B[D], (what, against, B[D])
    if D == 1:
        assert np.abs(got[0]).max() <= 2e-6, (what, np.abs(got[0]).max())      # the empty sum: logsumexp_n 0 - log N


def test_chunk_cap_by_sample_blocks():
    """1025 sample blocks: the chunk count is capped at 2048 / 1025 = 1 where N = CHUNK + 1 takes two with fewer samples.  D = 1;
    the fp64 restatement of this size runs in torch on the device."""
    N, S = L + 1, 262400
    mean, logvar, rows, eps = (t.numpy() for t in decomp_ref.clustered_posteriors(N, 1, S, seed=77))
    z = R.sample_z(mean, logvar, rows, eps)
    got, H = run_loo(mean, logvar, z)
    z64, m64, l64 = _dev(z, torch.float64), _dev(mean, torch.float64), _dev(logvar, torch.float64)
    ref = torch.cat([torch.logsumexp(decomp_ref.log_density(z64[s0:s0 + 8192], m64.t(), l64.t()), 1) - math.log(N)
                     for s0 in range(0, S, 8192)]).cpu().numpy()
    b = R.tolerance_multiple(run_joint(mean, logvar, z), ref)
    mult = R.tolerance_multiple(got[1], ref)
    print("cap: row 1 err / tol %.3f (shipped kernel %.3f); |row 0| max %.3g" % (mult, b, np.abs(got[0]).max()))
    assert mult <= max(1.0, 2 * b) and np.abs(got[0]).max() <= 2e-6
    assert abs(H[1] + ref.mean()) <= max(1.0, 2 * b) * (2e-6 * abs(ref.mean()) + 2e-6) and abs(H[0]) <= 2e-6


# ---- 2. degenerate samples, determinism -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,S", [(L + 1, 10, 257), (7, 17, 257)])
def test_far_sample_gives_minus_inf_where_every_remaining_dimension_is_far_and_never_nan(N, D, S):
    mean, logvar, rows, eps, z, ref = problem(N, D, S, "broad")
    plain, Hplain = run_loo(mean, logvar, z)
    s0, k = 33, 4
    # (a) 1e4 standard deviations from every data point in dimension k: about -5e7 in fp32 and in fp64 alike -- finite, and held
    # to the reference like any other sample
    far = z.copy()
    far[s0, k] = mean[:, k].max() + 1e4 * math.exp(0.5 * logvar[:, k].max())
    ref_far = R.loo_logq(far, mean, logvar)
    got, H = run_loo(mean, logvar, far)
    B, b = bounds(mean, logvar, far, ref_far, "broad")
    assert np.isfinite(got).all() and np.isfinite(H).all()
    assert (ref_far[np.arange(D + 1) != k, s0] < -1e7).all() and ref_far[k, s0] > -1e3
    for i in range(D + 1):
        assert R.tolerance_multiple(got[i], ref_far[i]) <= B[i], (i, B[i])
    # (b) so far that the square overflows fp32: every density that holds dimension k is -inf (as torch.logsumexp gives it), the
    # row that leaves k out is what it was, bit for bit; so is every other sample; nothing is NaN.  N = CHUNK + 1 and N = 7 end
    # their chunks in padding records, whose iv must not turn the infinite square into NaN.
    far = z.copy()
    far[s0, k] = 1e25
    got, H = run_loo(mean, logvar, far)
    assert not np.isnan(got).any() and not np.isnan(H).any()
    others = np.arange(D + 1) != k
    assert (got[others, s0] == -np.inf).all() and got[k, s0] == plain[k, s0] and np.isfinite(got[k, s0])
    keep = np.arange(S) != s0
    assert np.array_equal(got[:, keep], plain[:, keep])
    assert (H[others] == np.inf).all() and H[k] == Hplain[k]
    # ... and with ONE data point as far in the same dimension, the sample has that one finite density in every row
    mean2 = mean.copy()
    mean2[N - 1, k] = 1e25
    got2, _ = run_loo(mean2, logvar, far)
    ref2 = R.loo_logq(far[s0:s0 + 1].astype(np.float64), mean2, logvar)[:, 0]
    assert np.isfinite(ref2).all() and not np.isnan(got2).any()
    assert R.tolerance_multiple(got2[:, s0], ref2) <= 1.0, (got2[:, s0], ref2)


@pytest.mark.parametrize("N,D,S", [(L + 1, 10, 257), (7, 17, 257), (7, 1, 1)])
def test_same_bits_twice_and_on_a_second_stream_with_a_poisoned_workspace(N, D, S):
    mean, logvar, rows, eps, z, ref = problem(N, D, S, "sharp")
    a, Ha = run_loo(mean, logvar, z, ws_fill=0.0)
    b, Hb = run_loo(mean, logvar, z, ws_fill=0.0)
    assert a.tobytes() == b.tobytes() and Ha.tobytes() == Hb.tobytes()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c, Hc = run_loo(mean, logvar, z, st=side.cuda_stream, ws_fill=float("nan"))
    assert a.tobytes() == c.tobytes() and Ha.tobytes() == Hc.tobytes()


# ---- 3. dvae_sep_cond_terms -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 257])
@pytest.mark.parametrize("D", [1, 10, 17])
def test_cond_terms_vs_fp64(D, S):
    N = 300
    mean, logvar, rows, eps = (t.numpy() for t in decomp_ref.clustered_posteriors(N, D, S, seed=5 * D + S, logvar_range=(-10.0, 1.0)))
    ref, mean_abs = R.cond_terms(eps, logvar, rows)
    out = torch.full((D,), float("nan"), dtype=torch.float64, device=DEV)
    ed, ld, rd = _dev(eps), _dev(logvar), _dev(rows, torch.int64)
    _seplib.call("dvae_sep_cond_terms", ed.data_ptr(), ld.data_ptr(), rd.data_ptr(), N, D, S, out.data_ptr(), stream())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    bound = 8 * S * 2.0 ** -53 * mean_abs + 1e-6 * np.abs(ref)
    print("cond D%d S%d: max err %.3g, of the fp64 part of the bound %.3g" % (D, S, np.abs(got - ref).max(),
                                                                           (np.abs(got - ref) / (8 * S * 2.0 ** -53 * mean_abs)).max()))
    assert np.isfinite(got).all() and (np.abs(got - ref) <= bound).all(), (got, ref)


# ---- 4. memory contract -----------------------------------------------------------------------------------------------------------
def _sep_call(name):
    def fn(args):
        _seplib.call(name, *[a.ptr if isinstance(a, Guarded) else a for a in args])
    return fn


CONTRACT_SHAPES = [(7, 1, 1), (L + 1, 10, 257), (7, 17, 257), (64, MAX_D, 33)]


@pytest.mark.parametrize("N,D,S", CONTRACT_SHAPES)
def test_memory_contract_loo_logq(N, D, S):
    """Guards untouched, inputs unchanged, every output element written, bits equal to the run on plain tensors whatever the
    workspace and the surroundings hold (NaN at 256-byte alignment; -1e30 at the weakest alignment promised: the element's own)."""
    mean, logvar, rows, eps, z, _ = problem(N, D, S, "broad")
    nws = _seplib.lib().dvae_sep_loo_logq_ws_floats(N, D, S)

    def build(al):
        return [al.inp("z", z, align=4), al.inp("mean", mean, align=4), al.inp("logvar", logvar, align=4), N, D, S,
                al.ws("ws", (nws,), align=4), al.out("logq", (D + 1, S), align=4), al.out("H", (D + 1,), dtype=torch.float64, align=8),
                stream()]
    run_contract("dvae_sep_loo_logq", build, fn=_sep_call("dvae_sep_loo_logq"))


@pytest.mark.parametrize("N,D,S", CONTRACT_SHAPES)
def test_memory_contract_cond_terms(N, D, S):
    mean, logvar, rows, eps, z, _ = problem(N, D, S, "broad")

    def build(al):
        return [al.inp("eps", eps, align=4), al.inp("logvar", logvar, align=4), al.inp("rows", rows, align=8), N, D, S,
                al.out("H_cond_d", (D,), dtype=torch.float64, align=8), stream()]
    run_contract("dvae_sep_cond_terms", build, fn=_sep_call("dvae_sep_cond_terms"))


# ---- 5. the scores end to end -----------------------------------------------------------------------------------------------------
class _TableModel(torch.nn.Module):
    """A model whose encoder looks q(z|x) up in a table: image x is its row number."""

    def __init__(self, mean, logvar):
        super().__init__()
        self.latent_dim = mean.shape[1]
        self.register_buffer("mean", torch.from_numpy(np.ascontiguousarray(mean)))
        self.register_buffer("logvar", torch.from_numpy(np.ascontiguousarray(logvar)))
        self.modes = []

    def encoder(self, x):
        self.modes.append(self.training)
        idx = x.view(-1).long()
        return self.mean[idx], self.logvar[idx]


def _setup(mean, logvar, tmp_path):
    model = _TableModel(mean, logvar).train()
    n = mean.shape[0]
    loader = [(torch.arange(lo, min(lo + 10, n), dtype=torch.float32).view(-1, 1), None) for lo in range(0, n, 10)]
    ev = Evaluator(model, None, device=torch.device(DEV), logger=logging.getLogger("sep"), save_dir=str(tmp_path), is_progress_bar=False)
    return model, ev, loader


SCORE_KEYS = ("sepin", "wsepin", "sepin_at_k", "informativeness", "redundancy", "rho", "mi", "mi_loo", "dtc", "tc")


def _assert_scores(got, ref, what):
    atol = R.derived_atol(ref)
    assert set(got) == set(SCORE_KEYS) | {"H_z", "H_z_d", "H_loo", "H_cond_d", "n_samples", "n_data"}
    for k in ("H_z", "H_z_d", "H_loo", "H_cond_d"):
        np.testing.assert_allclose(got[k], ref[k], rtol=1e-5, atol=2e-6, err_msg=what + " " + k)
    for k in SCORE_KEYS:
        err = np.abs(np.asarray(got[k]) - np.asarray(ref[k])).max()
        print("%s %s: max err / atol %.3f" % (what, k, err / atol))
        assert err <= atol, (what, k, got[k], ref[k], atol)
    assert got["n_samples"] == ref["n_samples"] and got["n_data"] == ref["n_data"]
    json.dumps(got)
    return atol


def test_scores_of_a_product_aggregate_posterior(tmp_path):
    """Every combination of the digits present, jitter 0, logvar a function of (dimension, digit): q(z) is the product of its
    marginals -- no redundancy, no total correlation of either kind, sepin = informativeness."""
    mean, logvar, rows, eps = R.grid_table((4, 3, 2), 20, seed=2, product=True)
    model, ev, loader = _setup(mean, logvar, tmp_path)
    got = ev.compute_separability_scores(loader, sample_idx=torch.from_numpy(rows), eps=torch.from_numpy(eps))
    assert model.training and model.modes == [False] * 3                     # encoded in eval mode, mode restored
    ref = R.evaluation(R.sample_z(mean, logvar, rows, eps), eps, rows, mean, logvar)
    atol = _assert_scores(got, ref, "product")
    assert max(abs(v) for v in got["redundancy"]) <= atol and abs(got["dtc"]) <= atol and abs(got["tc"]) <= atol
    np.testing.assert_allclose(got["sepin"], got["informativeness"], rtol=0, atol=atol)
    assert got["sepin"] == [got["mi"] - v for v in got["mi_loo"]]
    np.testing.assert_allclose(got["sepin"], np.array(got["informativeness"]) - np.array(got["redundancy"]), rtol=0, atol=1e-12)


def test_scores_of_a_duplicated_column(tmp_path):
    """Column 1 a copy of column 0: whatever one of them tells about the image the other tells already."""
    mean, logvar, rows, eps = R.grid_table((4, 3, 2), 20, seed=3, product=True)
    dup = [0, 0, 1, 2]
    mean, logvar, eps = (np.ascontiguousarray(a[:, dup]) for a in (mean, logvar, eps))
    model, ev, loader = _setup(mean, logvar, tmp_path)
    got = ev.compute_separability_scores(loader, sample_idx=torch.from_numpy(rows), eps=torch.from_numpy(eps))
    ref = R.evaluation(R.sample_z(mean, logvar, rows, eps), eps, rows, mean, logvar)
    atol = _assert_scores(got, ref, "duplicate")
    print("duplicate: sepin %s informativeness %s atol %.3g" % (got["sepin"], got["informativeness"], atol))
    assert got["sepin"][0] <= atol and got["sepin"][1] <= atol and got["informativeness"][0] > 1
    assert got["sepin"][2] > 1 and got["sepin"][3] > 0.5                      # log 3 and log 2: the other two are told by nobody else


def test_same_seed_gives_the_samples_of_the_elbo_decomposition_and_the_log_file(tmp_path):
    mean, logvar, rows, eps, z, ref = problem(300, 7, 70, "broad")
    model, ev, loader = _setup(mean, logvar, tmp_path)
    cpu0, dev0 = torch.get_rng_state(), torch.cuda.get_rng_state()
    a = ev.compute_separability_scores(loader, n_samples=64, seed=3)
    b = ev.compute_separability_scores(loader, n_samples=64, seed=3)
    c = ev.compute_separability_scores(loader, n_samples=64, seed=4)
    elbo = ev.compute_elbo_decomposition(loader, n_samples=64, seed=3)
    assert torch.equal(torch.get_rng_state(), cpu0) and torch.equal(torch.cuda.get_rng_state(), dev0)
    assert a == b and a != c and model.training
    assert a["H_z_d"] == elbo["H_z_d"]                                        # bit for bit: the same samples, the same launch
    np.testing.assert_allclose(a["H_z"], elbo["H_z"], rtol=1e-5)
    np.testing.assert_allclose(a["tc"], elbo["tc"], rtol=0, atol=1e-5 * (abs(a["H_z"]) + sum(abs(h) for h in a["H_z_d"])))
    assert a["n_samples"] == 64 and a["n_data"] == 300 and len(a["sepin"]) == len(a["H_loo"]) == 7
    full = ev.compute_separability_scores(loader, n_samples=None, seed=1)
    assert full["n_samples"] == full["n_data"] == 300
    with pytest.raises(ValueError, match="exceeds"):
        ev.compute_separability_scores(loader, n_samples=301)
    # Evaluator.__call__: the file only on request, the return value the reference's
    assert not (tmp_path / "separability_scores.log").exists()
    assert ev(loader, is_losses=False, is_separability=True, n_samples_separability=64) == (None, None)
    assert json.load(open(tmp_path / "separability_scores.log")) == ev.compute_separability_scores(loader, n_samples=64)
    assert model.training and not any(model.modes)
