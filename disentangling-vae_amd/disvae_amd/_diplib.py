"""ctypes binding of libdvae_dip_hip.so (the C-ABI declared in include/dvae_dip_hip.h): the kernels behind the DIP-VAE-I / II
training losses (Kumar et al. 2018 in disentanglement_lib's form) -- the biased covariance of a batch of posterior means, the
regulariser that pulls it towards the identity, and its gradients with respect to the means and the log-variances.

A library of its own next to libdvae_hip.so (_lib.py) and the score libraries (one row each of build.py's TARGETS), loaded
lazily on first use.  As there, the library is the product: no CPU or PyTorch fallback, a missing shared object or symbol fails
loudly.  Unlike the score libraries this one takes part in the training step: models/losses.py issues its launches through
_lib.record_py, so a recorded plan re-issues them and a hipGraph captures them like any launch.
"""
import ctypes

from ._cabi import Binding, d as _d, i as _i, l as _l, p as _p

VERSION = 1                  # DVAE_DIP_VERSION
MAX_D = 128                  # DVAE_DIP_MAX_D: D above it is refused
THREADS = 256                # DVAE_DIP_THREADS: a workgroup
BLOCK_ROWS = 32              # DVAE_DIP_BLOCK_ROWS: rows of one trip; ceil(B / BLOCK_ROWS) workgroups ...
MAX_GROUPS = 64              # DVAE_DIP_MAX_GROUPS: ... at most; above BLOCK_ROWS * MAX_GROUPS rows a workgroup makes several trips

# name -> argtypes (all return int unless listed in _RESTYPE)
SIGNATURES = {
    "dvae_dip_version": [],
    "dvae_dip_last_error": [],
    "dvae_dip_ws_doubles": [_l, _i],
    "dvae_dip_moments": [_p, _p, _l, _i, _p, _p],
    "dvae_dip_grad": [_p, _p, _l, _i, _d, _d, _p, _p, _p, _p, _p, _p],
}
_RESTYPE = {"dvae_dip_last_error": ctypes.c_char_p, "dvae_dip_ws_doubles": ctypes.c_size_t}

_binding = Binding.for_library("dip", SIGNATURES, _RESTYPE, "DIP-VAE")
LIB_PATH = _binding.path       # DVAE_DIP_HIP_LIB overrides it


def groups(B):
    """(workgroups, rows of a chunk) of a batch of B rows: chunks_of(B, BLOCK_ROWS, MAX_GROUPS) of csrc/table_stats.h."""
    nb = min((B + BLOCK_ROWS - 1) // BLOCK_ROWS, MAX_GROUPS)
    chunk = (B + nb - 1) // nb
    return (B + chunk - 1) // chunk, chunk


def ws_doubles(B, D):
    """dvae_dip_ws_doubles for sizes in range, without a library load."""
    return groups(B)[0] * (2 * D + D * D)


def out_doubles(D):
    """`out` of dvae_dip_grad: R, R_od, R_d, then the D x D matrix C."""
    return 3 + D * D


def lib():
    """Load (once) and return the ctypes handle; raises if the library is absent."""
    return _binding.lib()


def call(name, *args):
    """Call an int-returning entry point, raise on a non-zero status."""
    _binding.call(lib(), name, *args)      # lib through the module: a test that replaces it intercepts this load too
