"""The one ctypes loader behind the bindings of every library but the training library's (_evallib.py, _scorelib.py, _infolib.py,
_irslib.py, _unsuplib.py, _udrlib.py, _dcilib.py, _diplib.py, _mmdlib.py, _seplib.py, _masslib.py, _saplib.py, _knnlib.py,
_lrlib.py, _weaklib.py, _semilib.py).

Each of those modules states what is its own -- its short name, mirrored constants, SIGNATURES, _RESTYPE -- and keeps a
module-level LIB_PATH and lib() / call() pair in front of one Binding.for_library(name, ...), which derives the rest from the
name: lib/libdvae_NAME_hip.so, its DVAE_NAME_HIP_LIB override and the dvae_NAME_last_error symbol.  _lib.py (the training
library, with plan recording) does not go through here.
"""
import ctypes
import os

from ._lib import DvaeHipError

_HERE = os.path.dirname(os.path.abspath(__file__))
# the argument types of the SIGNATURES tables
p, i, l, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_double      # noqa: E741


class Binding:
    def __init__(self, path, signatures, restype, last_error, kernels):
        """`last_error`: the library's dvae_*_last_error symbol; `kernels`: what the "not found" message calls its kernels."""
        self.path, self.signatures, self.restype, self.last_error, self.kernels = path, signatures, restype, last_error, kernels
        self.soname = "lib%s_hip.so" % last_error[:-len("_last_error")]
        self._lib = None

    @classmethod
    def for_library(cls, name, signatures, restype, kernels, subdir=""):
        """The binding of libdvae_NAME_hip.so in ../lib (`subdir`: in that sub-directory of it, build.py's EXTRA_DIR), or wherever
        the environment's DVAE_NAME_HIP_LIB says."""
        path = os.environ.get("DVAE_%s_HIP_LIB" % name.upper(), os.path.join(_HERE, "..", "lib", subdir, "libdvae_%s_hip.so" % name))
        return cls(path, signatures, restype, "dvae_%s_last_error" % name, kernels)

    def lib(self):
        """Load (once) and return the ctypes handle; raises if the library is absent."""
        if self._lib is None:
            path = os.path.abspath(self.path)
            if not os.path.exists(path):
                raise DvaeHipError(
                    "%s not found at %s -- build it with `python disentangling-vae_amd/build.py` "
                    "(there is no CPU / PyTorch fallback for the %s kernels)" % (self.soname, path, self.kernels))
            h = ctypes.CDLL(path)
            for name, argtypes in self.signatures.items():
                fn = getattr(h, name)  # AttributeError if the symbol is missing: fail loudly
                fn.argtypes = argtypes
                fn.restype = self.restype.get(name, ctypes.c_int)
            self._lib = h
        return self._lib

    def call(self, h, name, *args):
        """Call an int-returning entry point of the loaded handle `h`, raise on a non-zero status."""
        rc = getattr(h, name)(*args)
        if rc != 0:
            raise DvaeHipError("%s failed (%d): %s" % (name, rc, getattr(h, self.last_error)().decode()))
