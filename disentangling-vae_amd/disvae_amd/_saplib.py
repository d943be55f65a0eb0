"""ctypes binding of libdvae_sap_hip.so (the C-ABI declared in include/dvae_sap_hip.h): the kernels behind the discrete-factor
SAP score (Kumar et al. 2018; disentanglement_lib's sap_score.py with continuous_factors = False) -- every one-feature,
one-vs-rest squared-hinge SVM of a (latent, factor) pair fitted by Newton's method on the device, and the accuracy of the fits.

A library of its own next to libdvae_hip.so (_lib.py) and the other score libraries, built from build.py's MORE_TARGETS into
lib_more/ (a sibling of lib/) and loaded lazily on first use.  As there, the library is the product: no CPU or PyTorch fallback,
a missing shared object or symbol fails loudly.  Calls go straight to the library -- they are never recorded into a launch plan.
"""
import ctypes
import os

from ._cabi import Binding, d as _d, i as _i, l as _l, p as _p

VERSION = 1                  # DVAE_SAP_VERSION
MAX_FACTORS = 8              # DVAE_SAP_MAX_FACTORS: K above it is refused
MAX_CLASSES = 256            # DVAE_SAP_MAX_CLASSES: a factor with more classes present is refused
MAX_D = 65535                # DVAE_SAP_MAX_D
THREADS = 256                # DVAE_SAP_THREADS: one workgroup per problem
MAX_ROWS = 16384             # DVAE_SAP_MAX_ROWS: training rows of a fit (the column lives in LDS; there is no second path)
MAX_ITERATIONS = 64          # DVAE_SAP_MAX_ITERATIONS: Newton steps; a problem that needs more reports -1
MAX_HALVINGS = 30            # DVAE_SAP_MAX_HALVINGS: halvings of one step

# name -> argtypes (all return int unless listed in _RESTYPE)
SIGNATURES = {
    "dvae_sap_version": [],
    "dvae_sap_last_error": [],
    "dvae_sap_problems": [_p, _i],
    "dvae_sap_fit": [_p, _p, _p, _p, _l, _i, _i, _l, _d, _p, _p, _p],
    "dvae_sap_accuracy": [_p, _p, _p, _p, _l, _i, _i, _l, _p, _p, _p, _p],
}
_RESTYPE = {"dvae_sap_last_error": ctypes.c_char_p, "dvae_sap_problems": ctypes.c_long}

_binding = Binding.for_library("sap", SIGNATURES, _RESTYPE, "linear-SVM", subdir=os.path.join("..", "lib_more"))
LIB_PATH = _binding.path       # DVAE_SAP_HIP_LIB overrides it


def problems(n_classes):
    """The Python twin of dvae_sap_problems: problems per latent of factors with these numbers of classes present; -1 out of
    range."""
    n_classes = [int(c) for c in n_classes]
    if not 1 <= len(n_classes) <= MAX_FACTORS or not all(1 <= c <= MAX_CLASSES for c in n_classes):
        return -1
    return sum(c if c >= 3 else c - 1 for c in n_classes)


def host_classes(n_classes):
    """The HOST int32 array the entry points read n_classes from (keep it alive across the call)."""
    return (ctypes.c_int32 * len(n_classes))(*[int(c) for c in n_classes])


def lib():
    """Load (once) and return the ctypes handle; raises if the library is absent."""
    return _binding.lib()


def call(name, *args):
    """Call an int-returning entry point, raise on a non-zero status."""
    _binding.call(lib(), name, *args)      # lib through the module: a test that replaces it intercepts this load too
