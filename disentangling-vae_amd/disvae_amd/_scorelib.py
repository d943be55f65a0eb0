"""ctypes binding of libdvae_score_hip.so (the C-ABI declared in include/dvae_score_hip.h): the kernels behind the FactorVAE
and beta-VAE disentanglement scores.

A third library next to libdvae_hip.so (_lib.py) and libdvae_eval_hip.so (_evallib.py), loaded lazily on first use.  As there,
the library is the product: no CPU or PyTorch fallback, a missing shared object or symbol fails loudly.  Calls go straight to
the library -- they are never recorded into a launch plan (graph.py replays the training step only).
"""
import ctypes

from ._cabi import Binding, i as _i, l as _l, p as _p

VERSION = 1                  # DVAE_SCORE_VERSION
WAVE_MAX_L = 256             # DVAE_SCORE_WAVE_MAX_L: the longest group that one wave reduces (longer: a whole workgroup)
VOTE_LDS_BINS = 8192         # DVAE_SCORE_VOTE_LDS_BINS: the most K * D vote counters that are counted in LDS

# name -> argtypes (all return int unless listed in _RESTYPE)
SIGNATURES = {
    "dvae_score_version": [],
    "dvae_score_last_error": [],
    "dvae_score_group_var_ws_floats": [_l, _i, _l, _l],
    "dvae_score_group_var": [_p, _p, _l, _i, _l, _l, _p, _p, _p, _p],
    "dvae_score_pair_absdiff": [_p, _p, _p, _l, _i, _l, _l, _p, _p],
    "dvae_score_vote": [_p, _p, _p, _l, _i, _i, _p, _p, _p],
}
_RESTYPE = {"dvae_score_last_error": ctypes.c_char_p, "dvae_score_group_var_ws_floats": ctypes.c_size_t}

_binding = Binding.for_library("score", SIGNATURES, _RESTYPE, "score")
LIB_PATH = _binding.path       # DVAE_SCORE_HIP_LIB overrides it


def lib():
    """Load (once) and return the ctypes handle; raises if the library is absent."""
    return _binding.lib()


def call(name, *args):
    """Call an int-returning entry point, raise on a non-zero status."""
    _binding.call(lib(), name, *args)      # lib through the module: a test that replaces it intercepts this load too
