"""ctypes binding of libdvae_weak_hip.so (the C-ABI declared in include/dvae_weak_hip.h): the kernels behind the weakly-supervised
pair losses Ada-GVAE / Ada-ML-VAE (Locatello et al. 2020; disentanglement_lib's weak_vae.py) -- the adaptive group posterior of a
batch of image pairs on the interleaved [rows, 2 D] output of mu_logvar_gen, and its backward pass.

A library of its own next to libdvae_hip.so (_lib.py), the score libraries and the two other loss plugins, built from build.py's
SCORE_TARGETS into lib_scores/ (a sibling of lib/) and loaded lazily on first use.  As there, the library is the product: no CPU
or PyTorch fallback, a missing shared object or symbol fails loudly.  Like _diplib and _mmdlib it takes part in the training
step: models/losses.py issues its launches through _lib.record_py, so a recorded plan re-issues them and a hipGraph captures
them like any launch.
"""
import ctypes
import os

from ._cabi import Binding, i as _i, l as _l, p as _p

VERSION = 1                  # DVAE_WEAK_VERSION
MAX_D = 64                   # DVAE_WEAK_MAX_D: the mask of a pair is one 64-bit word; D above it is refused
MAX_PAIRS = 1 << 24          # DVAE_WEAK_MAX_PAIRS: pairs above it are refused
GVAE, MLVAE = 0, 1           # DVAE_WEAK_GVAE, DVAE_WEAK_MLVAE: the `kind` argument
KINDS = {"gvae": GVAE, "mlvae": MLVAE}
THREADS = 256                # DVAE_WEAK_THREADS: a workgroup

# name -> argtypes (all return int unless listed in _RESTYPE)
SIGNATURES = {
    "dvae_weak_version": [],
    "dvae_weak_last_error": [],
    "dvae_weak_aggregate_fwd": [_p, _l, _i, _i, _p, _p, _p, _p],
    "dvae_weak_aggregate_bwd": [_p, _p, _l, _i, _i, _p, _p],
}
_RESTYPE = {"dvae_weak_last_error": ctypes.c_char_p}

_binding = Binding.for_library("weak", SIGNATURES, _RESTYPE, "pair-aggregation", subdir=os.path.join("..", "lib_scores"))
LIB_PATH = _binding.path       # DVAE_WEAK_HIP_LIB overrides it


def group(D):
    """Lanes of a pair in the forward launch: D rounded up to a power of two (one wave holds 64 // group(D) pairs)."""
    g = 1
    while g < int(D):
        g *= 2
    return g


def lib():
    """Load (once) and return the ctypes handle; raises if the library is absent."""
    return _binding.lib()


def call(name, *args):
    """Call an int-returning entry point, raise on a non-zero status."""
    _binding.call(lib(), name, *args)      # lib through the module: a test that replaces it intercepts this load too
