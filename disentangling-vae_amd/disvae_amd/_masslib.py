"""ctypes binding of libdvae_mass_hip.so (the C-ABI declared in include/dvae_mass_hip.h): the kernels behind the factor-based
interpretability scores RMIG / JEMMIG (Do & Tran 2020), MIG-sup (Li et al. 2020) and DCIMIG (Sepliarskaia et al. 2019) -- the
posterior q(z_d | x) of every selected row integrated over fixed bins and summed per value of every factor of variation.

A library of its own next to libdvae_hip.so (_lib.py) and the other score libraries, built from build.py's EXTRA_TARGETS into
lib/ext/ and loaded lazily on first use.  As there, the library is the product: no CPU or PyTorch fallback, a missing shared
object or symbol fails loudly.  Calls go straight to the library -- they are never recorded into a launch plan.
"""
import ctypes

from ._cabi import Binding, i as _i, l as _l, p as _p

VERSION = 1                  # DVAE_MASS_VERSION
MAX_FACTORS = 8              # DVAE_MASS_MAX_FACTORS: K above it is refused
MAX_BINS = 256               # DVAE_MASS_MAX_BINS: n_bins above it is refused
WAVE_BINS = 63               # DVAE_MASS_WAVE_BINS: bins owned by one wave; a workgroup is ceil(n_bins / WAVE_BINS) waves
BLOCK_ROWS = 256             # DVAE_MASS_BLOCK_ROWS: rows of one chunk (one workgroup per chunk, latent and column group),
MAX_CHUNKS = 128             # DVAE_MASS_MAX_CHUNKS: until that many chunks are reached; then the chunks grow
TRIP_ROWS = 64               # DVAE_MASS_TRIP_ROWS: rows a workgroup loads at once
LDS_DOUBLES = 20000          # DVAE_MASS_LDS_DOUBLES: the most accumulators (n_bins per column) of one workgroup

# name -> argtypes (all return int unless listed in _RESTYPE)
SIGNATURES = {
    "dvae_mass_version": [],
    "dvae_mass_last_error": [],
    "dvae_mass_ws_doubles": [_l, _i, _i, _l, _i, _l],
    "dvae_mass_joint": [_p, _p, _p, _p, _p, _l, _i, _i, _l, _i, _l, _p, _p, _p],
}
_RESTYPE = {"dvae_mass_last_error": ctypes.c_char_p, "dvae_mass_ws_doubles": ctypes.c_size_t}

_binding = Binding.for_library("mass", SIGNATURES, _RESTYPE, "posterior-mass", subdir="ext")
LIB_PATH = _binding.path       # DVAE_MASS_HIP_LIB overrides it


def chunks(S):
    """(number of chunks, rows per chunk) the S selected rows are cut into: the library's chunks_of."""
    n = min(-(-S // BLOCK_ROWS), MAX_CHUNKS)
    rows = -(-S // n)
    return -(-S // rows), rows


def column_groups(n_bins, sum_sizes):
    """(number of column groups, columns per group): one group while n_bins * sum_sizes accumulators fit LDS_DOUBLES."""
    fit = LDS_DOUBLES // n_bins
    cols = -(-sum_sizes // -(-sum_sizes // fit))
    return -(-sum_sizes // cols), cols


def ws_doubles(N, D, K, S, n_bins, sum_sizes):
    """The Python twin of dvae_mass_ws_doubles: one [D, sum_sizes, n_bins] table per chunk; 0 for sizes out of range."""
    if S <= 0:
        S = N
    ok = 0 < N <= 2000000000 and 0 < D <= 16384 and 0 < K <= MAX_FACTORS and 0 < S <= 2000000000 and 1 <= n_bins <= MAX_BINS \
        and K <= sum_sizes <= 2000000000 and D * n_bins * sum_sizes <= 2147483647
    return chunks(S)[0] * D * n_bins * sum_sizes if ok else 0


def lib():
    """Load (once) and return the ctypes handle; raises if the library is absent."""
    return _binding.lib()


def call(name, *args):
    """Call an int-returning entry point, raise on a non-zero status."""
    _binding.call(lib(), name, *args)      # lib through the module: a test that replaces it intercepts this load too
