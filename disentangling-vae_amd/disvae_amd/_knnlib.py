"""ctypes binding of libdvae_knn_hip.so (the C-ABI declared in include/dvae_knn_hip.h): the kernels behind the binning-free
mutual-information scores -- the k-nearest-neighbour estimator of Ross 2014 (scikit-learn's _compute_mi_cd) between every latent
and every discrete factor of variation: a sort of each latent column and, per (latent, factor), the neighbour counts and the
three digamma sums, all in the LDS of one workgroup.

A library of its own next to libdvae_hip.so (_lib.py) and the other score libraries, built from build.py's SCORE_TARGETS into
lib_scores/ (a sibling of lib/) and loaded lazily on first use.  As there, the library is the product: no CPU or PyTorch fallback,
a missing shared object or symbol fails loudly.  Calls go straight to the library -- they are never recorded into a launch plan.
"""
import ctypes
import os

from ._cabi import Binding, i as _i, l as _l, p as _p

VERSION = 1                  # DVAE_KNN_VERSION
MAX_FACTORS = 8              # DVAE_KNN_MAX_FACTORS: K above it is refused
MAX_CLASSES = 256            # DVAE_KNN_MAX_CLASSES: a factor with more values is refused
MAX_NEIGHBORS = 64           # DVAE_KNN_MAX_NEIGHBORS: n_neighbors above it is refused
MAX_D = 65535                # DVAE_KNN_MAX_D
MAX_ROWS = 16384             # DVAE_KNN_MAX_ROWS: selected rows (a column lives in LDS; there is no second path)
SORT_THREADS = 1024          # DVAE_KNN_SORT_THREADS: one workgroup per latent column
SORT_ROW_BYTES = 8           # DVAE_KNN_SORT_ROW_BYTES: LDS per row of the column padded to a power of two
MI_THREADS = 512             # DVAE_KNN_MI_THREADS: one workgroup per (latent, factor)
MI_ROW_BYTES = 9             # DVAE_KNN_MI_ROW_BYTES: LDS per selected row
MI_FIXED_BYTES = 11520       # DVAE_KNN_MI_FIXED_BYTES: LDS of the tables besides

# name -> argtypes (all return int unless listed in _RESTYPE)
SIGNATURES = {
    "dvae_knn_version": [],
    "dvae_knn_last_error": [],
    "dvae_knn_ws_bytes": [_l, _i, _l],
    "dvae_knn_sort": [_p, _p, _l, _i, _l, _p, _p],
    "dvae_knn_mi": [_p, _p, _l, _i, _i, _l, _i, _p, _p, _p, _p, _p, _p, _p],
}
_RESTYPE = {"dvae_knn_last_error": ctypes.c_char_p, "dvae_knn_ws_bytes": ctypes.c_size_t}

_binding = Binding.for_library("knn", SIGNATURES, _RESTYPE, "k-NN mutual-information", subdir=os.path.join("..", "lib_scores"))
LIB_PATH = _binding.path       # DVAE_KNN_HIP_LIB overrides it


def lds_bytes(n_rows):
    """(bytes of LDS of a dvae_knn_sort workgroup, of a dvae_knn_mi workgroup) for n_rows selected rows: the header's plan."""
    padded = 1
    while padded < int(n_rows):
        padded *= 2
    return SORT_ROW_BYTES * padded, MI_ROW_BYTES * int(n_rows) + MI_FIXED_BYTES


def host_sizes(lat_sizes):
    """The HOST int32 array dvae_knn_mi reads lat_sizes from (keep it alive across the call)."""
    return (ctypes.c_int32 * len(lat_sizes))(*[int(c) for c in lat_sizes])


def lib():
    """Load (once) and return the ctypes handle; raises if the library is absent."""
    return _binding.lib()


def call(name, *args):
    """Call an int-returning entry point, raise on a non-zero status."""
    _binding.call(lib(), name, *args)      # lib through the module: a test that replaces it intercepts this load too
