"""ctypes binding of libdvae_udr_hip.so (the C-ABI declared in include/dvae_udr_hip.h): the kernels behind the unsupervised
disentanglement ranking (Duan et al. 2020) -- the tie-averaged rank of every element of a table of posterior means within its
column (a segmented radix sort) and the mean KL divergence of every latent dimension from the prior.

A seventh library next to libdvae_hip.so (_lib.py), libdvae_eval_hip.so (_evallib.py), libdvae_score_hip.so (_scorelib.py),
libdvae_info_hip.so (_infolib.py), libdvae_irs_hip.so (_irslib.py) and libdvae_unsup_hip.so (_unsuplib.py), loaded lazily on first
use.  As there, the library is the product: no CPU or PyTorch fallback, a missing shared object or symbol fails loudly.  Calls go
straight to the library -- they are never recorded into a launch plan (graph.py replays the training step only).
"""
import ctypes

from ._cabi import Binding, i as _i, l as _l, p as _p

VERSION = 1                  # DVAE_UDR_VERSION
MAX_D = 64                   # DVAE_UDR_MAX_D: D above it is refused
MAX_ROWS = 1 << 23           # DVAE_UDR_MAX_ROWS: the ranks refuse more selected rows (half-integer ranks stay exact in fp32)
SMALL_ROWS = 2048            # DVAE_UDR_SMALL_ROWS: up to that many rows one workgroup sorts a column in LDS
CHUNK_ROWS = 2048            # DVAE_UDR_CHUNK_ROWS: above, rows of one workgroup of a radix pass,
MAX_CHUNKS = 256             # DVAE_UDR_MAX_CHUNKS: until that many chunks (per column) are reached; then the chunks grow
KL_BLOCK_ROWS = 64           # DVAE_UDR_KL_BLOCK_ROWS: rows one thread of the KL pass adds in order,
KL_MAX_CHUNKS = 4096         # DVAE_UDR_KL_MAX_CHUNKS: until that many chunks are reached; then they grow

# name -> argtypes (all return int unless listed in _RESTYPE)
SIGNATURES = {
    "dvae_udr_version": [],
    "dvae_udr_last_error": [],
    "dvae_udr_ranks_ws_floats": [_l, _i, _l],
    "dvae_udr_kl_dims_ws_floats": [_l, _i, _l],
    "dvae_udr_ranks": [_p, _p, _l, _i, _l, _p, _p, _p],
    "dvae_udr_kl_dims": [_p, _p, _p, _l, _i, _l, _p, _p, _p],
}
_RESTYPE = {"dvae_udr_last_error": ctypes.c_char_p, "dvae_udr_ranks_ws_floats": ctypes.c_size_t,
            "dvae_udr_kl_dims_ws_floats": ctypes.c_size_t}

_binding = Binding.for_library("udr", SIGNATURES, _RESTYPE, "ranking")
LIB_PATH = _binding.path       # DVAE_UDR_HIP_LIB overrides it


def lib():
    """Load (once) and return the ctypes handle; raises if the library is absent."""
    return _binding.lib()


def call(name, *args):
    """Call an int-returning entry point, raise on a non-zero status."""
    _binding.call(lib(), name, *args)      # lib through the module: a test that replaces it intercepts this load too
