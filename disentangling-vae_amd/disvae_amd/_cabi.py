"""The one ctypes loader behind the score libraries' bindings (_evallib.py, _scorelib.py, _infolib.py, _irslib.py, _unsuplib.py).

Each of those modules states what is its own -- path, mirrored constants, SIGNATURES, _RESTYPE -- and keeps a module-level
lib() / call() pair in front of one Binding.  _lib.py (the training library, with plan recording) does not go through here.
"""
import ctypes
import os

from ._lib import DvaeHipError


class Binding:
    def __init__(self, path, signatures, restype, last_error, kernels):
        """`last_error`: the library's dvae_*_last_error symbol; `kernels`: what the "not found" message calls its kernels."""
        self.path, self.signatures, self.restype, self.last_error, self.kernels = path, signatures, restype, last_error, kernels
        self.soname = "lib%s_hip.so" % last_error[:-len("_last_error")]
        self._lib = None

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
