"""ctypes binding of libvboc_pool.so (include/vboc_pool.h): the pool side of the AL loop on the device - the
classifier's entropy over the unlabeled pool, the top-B selection with the pool's compaction, the guess network's
trajectories, and the RMSE march of the held-out states under the classifier.

`build()` compiles vboc_amd/csrc/pool.hip for gfx950 in-tree; `load()` raises when the library is missing (CPU runs
use learn.PoolScorer's torch / NumPy path explicitly).
"""
import ctypes
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libvboc_pool.so")
SRC = os.path.join(HERE, "csrc", "pool.hip")
EXPORTS = ("vboc_pool_create", "vboc_pool_destroy", "vboc_pool_set_classifier", "vboc_pool_set_guess",
           "vboc_pool_entropy", "vboc_pool_boundary", "vboc_pool_select", "vboc_pool_guess", "vboc_pool_last_error")
EARG, EHIP, EUNSUPPORTED = -1, -2, -3
MAX_HIDDEN, MAX_OUTPUTS = 512, 640


class PoolError(RuntimeError):
    def __init__(self, msg, code=None):
        super().__init__(msg)
        self.code = code


def build(verbose=False):
    # -ffp-contract=off: the kernels write every fma out; `out * std + mean` must stay a multiply and an add
    cmd = ["hipcc", "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-O3", "-ffp-contract=off", "-shared", SRC, "-o",
           LIB_PATH]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return LIB_PATH


_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PoolError(f"{LIB_PATH} not built - run __graft_entry__.build()")
    lib = ctypes.CDLL(LIB_PATH)
    for name in EXPORTS:
        getattr(lib, name)
    vp, ll, f = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_float
    lib.vboc_pool_last_error.restype = ctypes.c_char_p
    lib.vboc_pool_create.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(vp)]
    lib.vboc_pool_destroy.argtypes = [vp]
    lib.vboc_pool_set_classifier.argtypes = [vp] + [vp] * 6 + [vp]
    lib.vboc_pool_set_guess.argtypes = [vp, ctypes.c_int] + [vp] * 6 + [vp]
    lib.vboc_pool_entropy.argtypes = [vp, vp, ll, f, f, vp, vp, vp, vp]
    lib.vboc_pool_boundary.argtypes = [vp, vp, ctypes.c_int, f, f, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp]
    lib.vboc_pool_select.argtypes = [vp, vp, vp, ll, ll, ctypes.c_int, vp, vp, vp, ctypes.POINTER(f), vp]
    lib.vboc_pool_guess.argtypes = [vp, vp, ll, ctypes.c_int, f, f, vp, vp]
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        raise PoolError(f"vboc_pool error {rc}: {load().vboc_pool_last_error().decode()}", rc)


def supported(inputs, hidden, outputs=None):
    """The shapes pool.hip implements; `outputs` is the guess network's inputs * N (None: the classifier alone)."""
    ok = inputs in (2, 4, 6) and 1 <= hidden <= MAX_HIDDEN
    if outputs is not None:
        ok = ok and inputs <= outputs <= MAX_OUTPUTS and outputs % inputs == 0
    return ok
