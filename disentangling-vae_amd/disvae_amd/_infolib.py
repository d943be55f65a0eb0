"""ctypes binding of libdvae_info_hip.so (the C-ABI declared in include/dvae_info_hip.h): the kernels behind the discretised MIG,
modularity and SAP scores -- centred moments and joint histograms of the table of posterior means against the factors.

A fourth library next to libdvae_hip.so (_lib.py), libdvae_eval_hip.so (_evallib.py) and libdvae_score_hip.so (_scorelib.py),
loaded lazily on first use.  As there, the library is the product: no CPU or PyTorch fallback, a missing shared object or symbol
fails loudly.  Calls go straight to the library -- they are never recorded into a launch plan (graph.py replays the training
step only).
"""
import ctypes

from ._cabi import Binding, i as _i, l as _l, p as _p

VERSION = 1                  # DVAE_INFO_VERSION
MAX_FACTORS = 8              # DVAE_INFO_MAX_FACTORS: K above it is refused
MAX_BINS = 64                # DVAE_INFO_MAX_BINS: n_bins above it is refused
ROW_LANES_NARROW, ROW_LANES_MID, ROW_LANES_WAVE = 4, 16, 64   # DVAE_INFO_ROW_LANES_*: lanes per row of the moments pass, by D
MOMENTS_BLOCK_ROWS = 1024    # DVAE_INFO_MOMENTS_BLOCK_ROWS: rows of one workgroup of the moments pass ...
HIST_BLOCK_ROWS = 4096       # DVAE_INFO_HIST_BLOCK_ROWS: ... and of the histogram pass,
MAX_BLOCKS = 1024            # DVAE_INFO_MAX_BLOCKS: until that many workgroups (per latent) are reached; then the chunks grow
HIST_LDS_INTS = 8192         # DVAE_INFO_HIST_LDS_INTS: the most n_bins * sum(lat_sizes) counters that are kept in LDS

# name -> argtypes (all return int unless listed in _RESTYPE)
SIGNATURES = {
    "dvae_info_version": [],
    "dvae_info_last_error": [],
    "dvae_info_moments_ws_floats": [_l, _i, _i, _l],
    "dvae_info_hist_ws_floats": [_l, _i, _i, _l, _i, _l],
    "dvae_info_moments": [_p, _p, _p, _l, _i, _i, _l, _p, _p, _p, _p, _p, _p, _p, _p, _p],
    "dvae_info_joint_hist": [_p, _p, _p, _p, _l, _i, _i, _l, _i, _l, _p, _p, _p],
}
_RESTYPE = {"dvae_info_last_error": ctypes.c_char_p, "dvae_info_moments_ws_floats": ctypes.c_size_t,
            "dvae_info_hist_ws_floats": ctypes.c_size_t}

_binding = Binding.for_library("info", SIGNATURES, _RESTYPE, "information-score")
LIB_PATH = _binding.path       # DVAE_INFO_HIP_LIB overrides it


def lib():
    """Load (once) and return the ctypes handle; raises if the library is absent."""
    return _binding.lib()


def call(name, *args):
    """Call an int-returning entry point, raise on a non-zero status."""
    _binding.call(lib(), name, *args)      # lib through the module: a test that replaces it intercepts this load too
