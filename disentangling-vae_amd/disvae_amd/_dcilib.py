"""ctypes binding of libdvae_dci_hip.so (the C-ABI declared in include/dvae_dci_hip.h): the kernels behind the DCI scores
(Eastwood & Williams 2018 in disentanglement_lib's form) -- gradient-boosted depth-3 regression trees, scikit-learn's
GradientBoostingClassifier with default arguments restated, fitted on a table of posterior means where it lies; their
impurity-based feature importances and their raw scores on held-out rows.

A library of its own next to libdvae_hip.so (_lib.py) and the other score libraries (one row each of build.py's TARGETS), loaded
lazily on first use.  As there, the library is the product: no CPU or PyTorch fallback, a missing shared object or symbol fails
loudly.  Calls go straight to the library -- they are never recorded into a launch plan.
"""
import ctypes

from ._cabi import Binding, d as _d, i as _i, l as _l, p as _p

VERSION = 1                  # DVAE_DCI_VERSION
MAX_D = 64                   # DVAE_DCI_MAX_D: D above it is refused
MAX_CLASSES = 256            # DVAE_DCI_MAX_CLASSES: more classes of a factor are refused
MAX_ROWS = 10240             # DVAE_DCI_MAX_ROWS: selected rows of a fit -- one workgroup holds a sorted column in LDS
MAX_STAGES = 1024            # DVAE_DCI_MAX_STAGES: stages of one call
THREADS = 1024               # DVAE_DCI_THREADS: a workgroup; thread t owns ceil(S / THREADS) consecutive rows / positions
ROW_LDS_BYTES = 13           # DVAE_DCI_ROW_LDS_BYTES: residual fp64, value fp32, node byte
LDS_SCRATCH = 4096           # DVAE_DCI_LDS_SCRATCH: the scan's and the reduction's wave records
NODES = 15                   # DVAE_DCI_NODES: a depth-3 tree in heap order
NODE_STATS = 5               # DVAE_DCI_NODE_STATS: threshold, value, n, sum r, sum r^2
LAUNCHES_PER_STAGE = 8       # DVAE_DCI_LAUNCHES_PER_STAGE
LDS_BYTES = 160 * 1024       # of a CDNA4 compute unit: ROW_LDS_BYTES * MAX_ROWS + LDS_SCRATCH stays within it

# name -> argtypes (all return int unless listed in _RESTYPE)
SIGNATURES = {
    "dvae_dci_version": [],
    "dvae_dci_last_error": [],
    "dvae_dci_trees": [_i],
    "dvae_dci_fit_ws_floats": [_l, _i, _l, _i, _i],
    "dvae_dci_fit": [_p, _p, _p, _p, _l, _i, _l, _i, _i, _d, _i, _p, _p, _p, _p, _p, _p, _p, _p],
    "dvae_dci_predict": [_p, _p, _l, _i, _l, _i, _i, _d, _p, _p, _p, _p],
}
_RESTYPE = {"dvae_dci_last_error": ctypes.c_char_p, "dvae_dci_fit_ws_floats": ctypes.c_size_t}

_binding = Binding.for_library("dci", SIGNATURES, _RESTYPE, "boosted-tree")
LIB_PATH = _binding.path       # DVAE_DCI_HIP_LIB overrides it


def trees(C):
    """Trees per stage and columns of the raw scores: C, or 1 for C <= 2 (dvae_dci_trees, without a library load)."""
    return 1 if C <= 2 else int(C)


def lib():
    """Load (once) and return the ctypes handle; raises if the library is absent."""
    return _binding.lib()


def call(name, *args):
    """Call an int-returning entry point, raise on a non-zero status."""
    _binding.call(lib(), name, *args)      # lib through the module: a test that replaces it intercepts this load too
