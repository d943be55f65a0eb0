"""ctypes binding of libdvae_eval_hip.so (the C-ABI declared in include/dvae_eval_hip.h): the evaluation-side kernels.

A second library next to libdvae_hip.so (_lib.py), loaded lazily on first use.  As there, the library is the product: no CPU
or PyTorch fallback, a missing shared object or symbol fails loudly.  Calls go straight to the library -- they are never
recorded into a launch plan (graph.py replays the training step only).
"""
import ctypes

from ._cabi import Binding, i as _i, l as _l, p as _p

VERSION = 1                  # DVAE_EVAL_VERSION
JOINT_CHUNK = 2048           # DVAE_EVAL_JOINT_CHUNK: data points per workgroup of the joint log-density kernel (at least)
JOINT_MAX_CHUNKS = 256       # DVAE_EVAL_JOINT_MAX_CHUNKS

# name -> argtypes (all return int unless listed in _RESTYPE)
SIGNATURES = {
    "dvae_eval_version": [],
    "dvae_eval_last_error": [],
    "dvae_eval_joint_logq_ws_floats": [_l, _i, _l],
    "dvae_eval_joint_logq": [_p, _p, _p, _l, _i, _l, _p, _p, _p, _p],
    "dvae_eval_sample_terms": [_p, _p, _p, _p, _l, _i, _l, _p, _p, _p, _p],
}
_RESTYPE = {"dvae_eval_last_error": ctypes.c_char_p, "dvae_eval_joint_logq_ws_floats": ctypes.c_size_t}

_binding = Binding.for_library("eval", SIGNATURES, _RESTYPE, "evaluation")
LIB_PATH = _binding.path       # DVAE_EVAL_HIP_LIB overrides it


def lib():
    """Load (once) and return the ctypes handle; raises if the library is absent."""
    return _binding.lib()


def call(name, *args):
    """Call an int-returning entry point, raise on a non-zero status."""
    _binding.call(lib(), name, *args)      # lib through the module: a test that replaces it intercepts this load too
