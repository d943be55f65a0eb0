"""ctypes binding of libdvae_mmd_hip.so (the C-ABI declared in include/dvae_mmd_hip.h): the kernels behind the InfoVAE / MMD-VAE
training loss (Zhao, Song & Ermon 2019; the regulariser of WAE-MMD) -- the unbiased maximum mean discrepancy between a batch of
latent samples and as many prior samples under an RBF or an inverse-multiquadric-sum kernel, and its gradient with respect to
the samples.

A library of its own next to libdvae_hip.so (_lib.py), the score libraries and libdvae_dip_hip.so, built from build.py's
PLUGIN_TARGETS and loaded lazily on first use.  As there, the library is the product: no CPU or PyTorch fallback, a missing
shared object or symbol fails loudly.  Like _diplib it takes part in the training step: models/losses.py issues its launches
through _lib.record_py, so a recorded plan re-issues them and a hipGraph captures them like any launch.
"""
import ctypes

from ._cabi import Binding, d as _d, i as _i, l as _l, p as _p

VERSION = 1                  # DVAE_MMD_VERSION
MAX_D = 128                  # DVAE_MMD_MAX_D: D above it is refused
MAX_B = 65536                # DVAE_MMD_MAX_B: B above it is refused
RBF, IMQ = 0, 1              # DVAE_MMD_RBF, DVAE_MMD_IMQ: the `kernel` argument
KERNELS = {"rbf": RBF, "imq": IMQ}
THREADS = 256                # DVAE_MMD_THREADS: a workgroup
ROWS = 16                    # DVAE_MMD_ROWS: rows of a tile; 2 ceil(B / ROWS) row tiles (z, then p)
COLS = 32                    # DVAE_MMD_COLS: columns of one trip; ceil(columns / COLS) chunks ...
MAX_CGROUPS = 8              # DVAE_MMD_MAX_CGROUPS: ... at most; above COLS * MAX_CGROUPS columns a workgroup makes several trips
IMQ_SCALES = (0.1, 0.2, 0.5, 1.0, 2.0, 5.0, 10.0)      # C_s = h s (WAE's sum of inverse multiquadrics)

# name -> argtypes (all return int unless listed in _RESTYPE)
SIGNATURES = {
    "dvae_mmd_version": [],
    "dvae_mmd_last_error": [],
    "dvae_mmd_ws_doubles": [_l, _i],
    "dvae_mmd_pairs": [_p, _p, _l, _i, _i, _d, _i, _p, _p],
    "dvae_mmd_finish": [_p, _p, _l, _i, _d, _p, _p, _p, _p, _p, _p],
}
_RESTYPE = {"dvae_mmd_last_error": ctypes.c_char_p, "dvae_mmd_ws_doubles": ctypes.c_size_t}

_binding = Binding.for_library("mmd", SIGNATURES, _RESTYPE, "InfoVAE MMD")
LIB_PATH = _binding.path       # DVAE_MMD_HIP_LIB overrides it
OUT_DOUBLES = 5                # `out` of dvae_mmd_finish: w MMD_u, MMD_u, S_zz, S_pp, S_zp


def _chunks(n):
    """(chunks, columns of a chunk) of n columns: chunks_of(n, COLS, MAX_CGROUPS) of csrc/table_stats.h."""
    nb = min((n + COLS - 1) // COLS, MAX_CGROUPS)
    chunk = (n + nb - 1) // nb
    return (n + chunk - 1) // chunk, chunk


def tiling(B):
    """(row tiles per table, (chunks, chunk) of a z tile's 2 B columns, (chunks, chunk) of a p tile's B columns)."""
    return (B + ROWS - 1) // ROWS, _chunks(2 * B), _chunks(B)


def ws_doubles(B, D):
    """dvae_mmd_ws_doubles for sizes in range, without a library load."""
    tiles, (gz, _), _ = tiling(B)
    return 4 * tiles * gz + B * gz * D


def lib():
    """Load (once) and return the ctypes handle; raises if the library is absent."""
    return _binding.lib()


def call(name, *args):
    """Call an int-returning entry point, raise on a non-zero status."""
    _binding.call(lib(), name, *args)      # lib through the module: a test that replaces it intercepts this load too
