"""ctypes binding of libdvae_lr_hip.so (the C-ABI declared in include/dvae_lr_hip.h): the kernels behind the linear-softmax probes
-- the multinomial logistic regression of the beta-VAE score, of explicitness and of InfoE (Hsu et al. 2023) fitted on the device
by a truncated Newton-CG iteration in fp64, one persistent workgroup per problem, and the evaluation of the fits.

A library of its own next to libdvae_hip.so (_lib.py) and the other score libraries, built from build.py's SCORE_TARGETS into
lib_scores/ (a sibling of lib/) and loaded lazily on first use.  As there, the library is the product: no CPU or PyTorch fallback,
a missing shared object or symbol fails loudly.  Calls go straight to the library -- they are never recorded into a launch plan.
"""
import ctypes
import os

from ._cabi import Binding, d as _d, i as _i, l as _l, p as _p

VERSION = 1                  # DVAE_LR_VERSION
MAX_ROWS = 16384             # DVAE_LR_MAX_ROWS: training rows of a fit
MAX_D = 64                   # DVAE_LR_MAX_D
MAX_CLASSES = 256            # DVAE_LR_MAX_CLASSES: classes of one problem
MAX_PROBLEMS = 8             # DVAE_LR_MAX_PROBLEMS: problems of one call (they share the features)
THREADS = 512                # DVAE_LR_THREADS: one workgroup per problem
FEATURE_TILE = 16            # DVAE_LR_FEATURE_TILE: features of a row held in registers at a time
CHUNK_ROWS = 64              # DVAE_LR_CHUNK_ROWS: the fewest rows of a chunk of a sum over the rows
PREDICT_THREADS = 128        # DVAE_LR_PREDICT_THREADS
MAX_ITERATIONS = 100         # DVAE_LR_MAX_ITERATIONS: Newton steps; a problem that needs more reports -1
MAX_CG = 400                 # DVAE_LR_MAX_CG: conjugate-gradient steps of one Newton step
MAX_HALVINGS = 30            # DVAE_LR_MAX_HALVINGS: halvings of one step

# name -> argtypes (all return int unless listed in _RESTYPE)
SIGNATURES = {
    "dvae_lr_version": [],
    "dvae_lr_last_error": [],
    "dvae_lr_ws_bytes": [_l, _i, _p, _i],
    "dvae_lr_fit": [_p, _p, _p, _p, _p, _l, _i, _i, _d, _d, _p, _p, _p, _p],
    "dvae_lr_predict": [_p, _p, _p, _p, _p, _l, _i, _i, _p, _p, _p, _p, _p, _p],
}
_RESTYPE = {"dvae_lr_last_error": ctypes.c_char_p, "dvae_lr_ws_bytes": ctypes.c_long}

_binding = Binding.for_library("lr", SIGNATURES, _RESTYPE, "softmax-regression", subdir=os.path.join("..", "lib_scores"))
LIB_PATH = _binding.path       # DVAE_LR_HIP_LIB overrides it


def chunks(n_rows, n_classes, dim):
    """(n_chunks, rows of a chunk) of a sum over n_rows rows of a problem with these sizes: the header's plan."""
    per = max(THREADS // (int(n_classes) * (int(dim) + 1)), 1)
    nb = min((int(n_rows) + CHUNK_ROWS - 1) // CHUNK_ROWS, per)
    chunk = (int(n_rows) + nb - 1) // nb
    return (int(n_rows) + chunk - 1) // chunk, chunk


def coef_sizes(n_classes, dim):
    """Values of `coef` per problem: C_q (D + 1)."""
    return [int(c) * (int(dim) + 1) for c in n_classes]


def host_classes(n_classes):
    """The HOST int32 array the entry points read n_classes from (keep it alive across the call)."""
    return (ctypes.c_int32 * len(n_classes))(*[int(c) for c in n_classes])


def lib():
    """Load (once) and return the ctypes handle; raises if the library is absent."""
    return _binding.lib()


def call(name, *args):
    """Call an int-returning entry point, raise on a non-zero status."""
    _binding.call(lib(), name, *args)      # lib through the module: a test that replaces it intercepts this load too
