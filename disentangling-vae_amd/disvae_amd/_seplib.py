"""ctypes binding of libdvae_sep_hip.so (the C-ABI declared in include/dvae_sep_hip.h): the kernels behind the SEPIN / WSEPIN
separability scores (Do & Tran 2020) -- the leave-one-out joint log-density of every latent dimension under the aggregate
posterior, the joint one from the same pass, and the conditional entropy per dimension.

A library of its own next to libdvae_hip.so (_lib.py) and the other score libraries, built from build.py's SCORE_PLUGIN_TARGETS
and loaded lazily on first use.  As there, the library is the product: no CPU or PyTorch fallback, a missing shared object or
symbol fails loudly.  Calls go straight to the library -- they are never recorded into a launch plan.
"""
import ctypes

from ._cabi import Binding, i as _i, l as _l, p as _p

VERSION = 1                  # DVAE_SEP_VERSION
MAX_D = 64                   # DVAE_SEP_MAX_D: D above it is refused
TEMPLATE_D = 16              # DVAE_SEP_TEMPLATE_D: up to it a kernel compiled for the width, above it the run-time-D kernel
GROUP = 16                   # DVAE_SEP_GROUP: rows of the [D + 1, S] result per workgroup of the run-time-D kernel (gridDim.z groups)
CHUNK = 2048                 # DVAE_SEP_CHUNK: data points per workgroup (at least)
MAX_CHUNKS = 256             # DVAE_SEP_MAX_CHUNKS

# name -> argtypes (all return int unless listed in _RESTYPE)
SIGNATURES = {
    "dvae_sep_version": [],
    "dvae_sep_last_error": [],
    "dvae_sep_loo_logq_ws_floats": [_l, _i, _l],
    "dvae_sep_loo_logq": [_p, _p, _p, _l, _i, _l, _p, _p, _p, _p],
    "dvae_sep_cond_terms": [_p, _p, _p, _l, _i, _l, _p, _p],
}
_RESTYPE = {"dvae_sep_last_error": ctypes.c_char_p, "dvae_sep_loo_logq_ws_floats": ctypes.c_size_t}

_binding = Binding.for_library("sep", SIGNATURES, _RESTYPE, "separability")
LIB_PATH = _binding.path       # DVAE_SEP_HIP_LIB overrides it


def lib():
    """Load (once) and return the ctypes handle; raises if the library is absent."""
    return _binding.lib()


def call(name, *args):
    """Call an int-returning entry point, raise on a non-zero status."""
    _binding.call(lib(), name, *args)      # lib through the module: a test that replaces it intercepts this load too
