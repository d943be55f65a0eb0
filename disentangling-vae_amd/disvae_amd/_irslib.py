"""ctypes binding of libdvae_irs_hip.so (the C-ABI declared in include/dvae_irs_hip.h): the kernels behind the interventional
robustness score -- the mean of every latent over every group of rows that share a (binned) factor value, and exact order
statistics of the absolute deviations from a centre per group.

A fifth library next to libdvae_hip.so (_lib.py), libdvae_eval_hip.so (_evallib.py), libdvae_score_hip.so (_scorelib.py) and
libdvae_info_hip.so (_infolib.py), loaded lazily on first use.  As there, the library is the product: no CPU or PyTorch fallback,
a missing shared object or symbol fails loudly.  Calls go straight to the library -- they are never recorded into a launch plan
(graph.py replays the training step only).
"""
import ctypes

from ._cabi import Binding, i as _i, l as _l, p as _p

VERSION = 1                  # DVAE_IRS_VERSION
MAX_FACTORS = 8              # DVAE_IRS_MAX_FACTORS: K above it is refused
MAX_GROUPS = 256             # DVAE_IRS_MAX_GROUPS: more groups of one factor are refused
MEANS_COLS = 16              # DVAE_IRS_MEANS_COLS: the means pass walks a row in pieces of that many floats
MEANS_BLOCK_ROWS = 1024      # DVAE_IRS_MEANS_BLOCK_ROWS: rows of one workgroup of the means pass ...
SELECT_BLOCK_ROWS = 4096     # DVAE_IRS_SELECT_BLOCK_ROWS: ... and of a selection pass,
MAX_BLOCKS = 512             # DVAE_IRS_MAX_BLOCKS: until that many chunks are reached; then the chunks grow
SELECT_LDS_GROUPS = 40       # DVAE_IRS_SELECT_LDS_GROUPS: groups of one factor whose digit histograms one workgroup keeps in LDS
SELECT_PASSES = 4            # DVAE_IRS_SELECT_PASSES: 8-bit passes of the radix select
MAX_PAIRS = 4194304          # DVAE_IRS_MAX_PAIRS: the most total_groups * D

# name -> argtypes (all return int unless listed in _RESTYPE)
SIGNATURES = {
    "dvae_irs_version": [],
    "dvae_irs_last_error": [],
    "dvae_irs_group_means_ws_floats": [_l, _i, _i, _l, _i],
    "dvae_irs_group_order_stats_ws_floats": [_l, _i, _i, _l, _i],
    "dvae_irs_group_means": [_p, _p, _p, _p, _p, _l, _i, _i, _l, _l, _i, _i, _p, _p, _p, _p],
    "dvae_irs_group_order_stats": [_p, _p, _p, _p, _p, _p, _p, _l, _i, _i, _l, _l, _i, _i, _p, _p, _p, _p, _p],
}
_RESTYPE = {"dvae_irs_last_error": ctypes.c_char_p, "dvae_irs_group_means_ws_floats": ctypes.c_size_t,
            "dvae_irs_group_order_stats_ws_floats": ctypes.c_size_t}

_binding = Binding.for_library("irs", SIGNATURES, _RESTYPE, "interventional-robustness")
LIB_PATH = _binding.path       # DVAE_IRS_HIP_LIB overrides it


def lib():
    """Load (once) and return the ctypes handle; raises if the library is absent."""
    return _binding.lib()


def call(name, *args):
    """Call an int-returning entry point, raise on a non-zero status."""
    _binding.call(lib(), name, *args)      # lib through the module: a test that replaces it intercepts this load too
