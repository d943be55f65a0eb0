"""ctypes binding of libdvae_unsup_hip.so (the C-ABI declared in include/dvae_unsup_hip.h): the kernels behind the label-free
scores (Gaussian total correlation, Gaussian Wasserstein correlation, mean pairwise mutual information of the discretised
latents) -- the D x D covariance of the table of posterior means and the joint histograms of every pair of its columns.

A sixth library next to libdvae_hip.so (_lib.py), libdvae_eval_hip.so (_evallib.py), libdvae_score_hip.so (_scorelib.py),
libdvae_info_hip.so (_infolib.py) and libdvae_irs_hip.so (_irslib.py), loaded lazily on first use.  As there, the library is the
product: no CPU or PyTorch fallback, a missing shared object or symbol fails loudly.  Calls go straight to the library -- they
are never recorded into a launch plan (graph.py replays the training step only).
"""
import ctypes

from ._cabi import Binding, i as _i, l as _l, p as _p

VERSION = 1                  # DVAE_UNSUP_VERSION
MAX_D = 64                   # DVAE_UNSUP_MAX_D: D above it is refused
MAX_BINS = 64                # DVAE_UNSUP_MAX_BINS: n_bins above it is refused
MOMENTS_BLOCK_ROWS = 1024    # DVAE_UNSUP_MOMENTS_BLOCK_ROWS: rows of one workgroup of the moments pass ...
HIST_BLOCK_ROWS = 4096       # DVAE_UNSUP_HIST_BLOCK_ROWS: ... and of the histogram pass,
MAX_BLOCKS = 1024            # DVAE_UNSUP_MAX_BLOCKS: until that many workgroups (per tile of pairs) are reached; then the chunks grow
MOMENTS_THREAD_SUMS = 9      # DVAE_UNSUP_MOMENTS_THREAD_SUMS: sums one thread of the moments pass keeps at most (256 threads)
HIST_LDS_INTS = 4096         # DVAE_UNSUP_HIST_LDS_INTS: the counters of one tile of pairs, n_bins^2 per pair, one pair at least

# name -> argtypes (all return int unless listed in _RESTYPE)
SIGNATURES = {
    "dvae_unsup_version": [],
    "dvae_unsup_last_error": [],
    "dvae_unsup_moments_ws_floats": [_l, _i, _l],
    "dvae_unsup_pair_hist_ws_floats": [_l, _i, _l, _i],
    "dvae_unsup_moments": [_p, _p, _l, _i, _l, _p, _p, _p, _p, _p, _p],
    "dvae_unsup_pair_hist": [_p, _p, _p, _l, _i, _l, _i, _p, _p, _p],
}
_RESTYPE = {"dvae_unsup_last_error": ctypes.c_char_p, "dvae_unsup_moments_ws_floats": ctypes.c_size_t,
            "dvae_unsup_pair_hist_ws_floats": ctypes.c_size_t}

_binding = Binding.for_library("unsup", SIGNATURES, _RESTYPE, "label-free score")
LIB_PATH = _binding.path       # DVAE_UNSUP_HIP_LIB overrides it


def lib():
    """Load (once) and return the ctypes handle; raises if the library is absent."""
    return _binding.lib()


def call(name, *args):
    """Call an int-returning entry point, raise on a non-zero status."""
    _binding.call(lib(), name, *args)      # lib through the module: a test that replaces it intercepts this load too
