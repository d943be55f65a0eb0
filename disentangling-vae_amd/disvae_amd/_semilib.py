"""ctypes binding of libdvae_semi_hip.so (the C-ABI declared in include/dvae_semi_hip.h): the kernels behind the semi-supervised
training loss S2-beta-VAE (Locatello et al. 2020, "Disentangling Factors of Variation Using Few Labels"; disentanglement_lib's
semi_supervised_vae.py) -- the supervised regulariser that ties latent k to factor k on the labelled rows of a batch, and its
gradient with respect to the posterior means.

A library of its own next to libdvae_hip.so (_lib.py), the score libraries and the three other loss plugins, built from build.py's
SCORE_TARGETS into lib_scores/ (a sibling of lib/) and loaded lazily on first use.  As there, the library is the product: no CPU
or PyTorch fallback, a missing shared object or symbol fails loudly.  Like _diplib, _mmdlib and _weaklib it takes part in the
training step: models/losses.py issues its launches through _lib.record_py, so a recorded plan re-issues them and a hipGraph
captures them like any launch.
"""
import ctypes
import os

from ._cabi import Binding, i as _i, l as _l, p as _p

VERSION = 1                  # DVAE_SEMI_VERSION
MAX_D = 64                   # DVAE_SEMI_MAX_D: D above it is refused
MAX_K = 8                    # DVAE_SEMI_MAX_K: more factors are refused
MAX_ROWS = 16384             # DVAE_SEMI_MAX_ROWS: more rows are refused
THREADS = 256                # DVAE_SEMI_THREADS: a workgroup
BLOCK_ROWS = 64              # DVAE_SEMI_BLOCK_ROWS: rows of one chunk; ceil(n / BLOCK_ROWS) workgroups
XENT, L2, COV = 0, 1, 2      # DVAE_SEMI_XENT, DVAE_SEMI_L2, DVAE_SEMI_COV: the `kind` argument
KINDS = {"xent": XENT, "l2": L2, "cov": COV}
SUM, MEAN = 0, 1             # DVAE_SEMI_SUM, DVAE_SEMI_MEAN: the `reduction` argument
REDUCTIONS = {"sum": SUM, "mean": MEAN}

# name -> argtypes (all return int unless listed in _RESTYPE)
SIGNATURES = {
    "dvae_semi_version": [],
    "dvae_semi_last_error": [],
    "dvae_semi_ws_doubles": [_l, _i, _i],
    "dvae_semi_partials": [_p, _i, _p, _l, _i, _i, _p, _p, _i, _p, _p],
    "dvae_semi_grad": [_p, _i, _p, _l, _i, _i, _p, _p, _i, _i, _p, _p, _p, _p, _p, _p],
}
_RESTYPE = {"dvae_semi_last_error": ctypes.c_char_p, "dvae_semi_ws_doubles": ctypes.c_size_t}

_binding = Binding.for_library("semi", SIGNATURES, _RESTYPE, "label-regulariser", subdir=os.path.join("..", "lib_scores"))
LIB_PATH = _binding.path       # DVAE_SEMI_HIP_LIB overrides it


def groups(n):
    """Workgroups (chunks of BLOCK_ROWS rows) of a batch of n rows."""
    return (int(n) + BLOCK_ROWS - 1) // BLOCK_ROWS


def rec_doubles(D, K):
    """One chunk's record in the workspace: n_lab, the value sum, then (cov) D + K column sums and the D x K cross sums."""
    return 2 + D + K + D * K


def ws_doubles(n, D, K):
    """dvae_semi_ws_doubles for sizes in range, without a library load."""
    return groups(n) * rec_doubles(D, K)


def out_doubles(D, K):
    """`out` of dvae_semi_grad: R, n_lab, then the D x K matrix C."""
    return 2 + D * K


def factor_table(lat_sizes, factors):
    """(sizes, strides) of the chosen factors of a data set that enumerates ``lat_sizes`` in row-major order, as two ctypes int64
    arrays: the HOST pointers the entry points take (keep them alive as long as a recorded launch may be re-issued)."""
    sizes = [int(s) for s in lat_sizes]
    strides = [1] * len(sizes)
    for j in range(len(sizes) - 2, -1, -1):
        strides[j] = strides[j + 1] * sizes[j + 1]
    arr = ctypes.c_int64 * len(factors)
    return arr(*[sizes[j] for j in factors]), arr(*[strides[j] for j in factors])


def lib():
    """Load (once) and return the ctypes handle; raises if the library is absent."""
    return _binding.lib()


def call(name, *args):
    """Call an int-returning entry point, raise on a non-zero status."""
    _binding.call(lib(), name, *args)      # lib through the module: a test that replaces it intercepts this load too
