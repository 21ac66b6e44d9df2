"""ctypes binding of libvboc_cls.so (include/vboc_cls.h): the HJR / AL classifier on the device - the BCE fit, the
classification of a candidate set and the RMSE march.

`build()` compiles vboc_amd/csrc/cls.hip for gfx950 in-tree; `load()` raises when the library is missing (CPU runs
use learn.ClsTrainer explicitly).
"""
import ctypes
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libvboc_cls.so")
SRC = os.path.join(HERE, "csrc", "cls.hip")
EXPORTS = ("vboc_cls_create", "vboc_cls_destroy", "vboc_cls_set_params", "vboc_cls_get_params", "vboc_cls_train",
           "vboc_cls_sample", "vboc_cls_train_split", "vboc_cls_sample_split", "vboc_cls_eval", "vboc_cls_boundary",
           "vboc_cls_last_error")
EUNSUPPORTED = -3


class ClsError(RuntimeError):
    pass


class ClsRun(ctypes.Structure):
    """vboc_cls_run_t"""
    _fields_ = [("F", ctypes.c_void_p), ("n", ctypes.c_longlong), ("ld", ctypes.c_int),
                ("it_max", ctypes.c_longlong), ("val0", ctypes.c_double), ("stop_val", ctypes.c_double),
                ("beta", ctypes.c_double), ("lr", ctypes.c_double), ("poll", ctypes.c_int), ("graphs", ctypes.c_int),
                ("iterations", ctypes.c_void_p), ("val", ctypes.c_void_p), ("launched", ctypes.c_void_p),
                ("kernel_ms", ctypes.c_void_p)]


def build(verbose=False):
    cmd = ["hipcc", "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-O3", "-shared", SRC, "-o", LIB_PATH]
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
        raise ClsError(f"{LIB_PATH} not built - run __graft_entry__.build()")
    lib = ctypes.CDLL(LIB_PATH)
    for name in EXPORTS:
        getattr(lib, name)
    vp, ll = ctypes.c_void_p, ctypes.c_longlong
    lib.vboc_cls_last_error.restype = ctypes.c_char_p
    lib.vboc_cls_create.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_ulonglong, ctypes.POINTER(vp)]
    lib.vboc_cls_destroy.argtypes = [vp]
    lib.vboc_cls_set_params.argtypes = [vp] + [vp] * 7
    lib.vboc_cls_get_params.argtypes = [vp, ctypes.c_int] + [vp] * 7
    lib.vboc_cls_train.argtypes = [vp, ctypes.POINTER(ClsRun), vp]
    lib.vboc_cls_sample.argtypes = [vp, ll, ctypes.c_int, vp, vp]
    lib.vboc_cls_train_split.argtypes = [vp, ctypes.POINTER(ClsRun), ll, vp]
    lib.vboc_cls_sample_split.argtypes = [vp, ll, ll, ctypes.c_int, vp, vp]
    lib.vboc_cls_eval.argtypes = [vp, vp, ll, ctypes.c_int, vp, vp, ctypes.POINTER(ll), vp]
    lib.vboc_cls_boundary.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float,
                                      ctypes.c_int, vp, vp, vp, vp]
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        raise ClsError(f"vboc_cls error {rc}: {load().vboc_cls_last_error().decode()}")


def supported(inputs, hidden, minibatch):
    return inputs in (2, 4, 6) and 65 <= hidden <= 128 and minibatch % 32 == 0 and 32 <= minibatch <= 4096


def fit_supported(inputs, hidden, minibatch):
    """The shapes the training step exists at: `supported`'s, and fit.hip's wide ones (the AL loop's 300 and 500),
    where the handle is a trainer only."""
    wide = (inputs == 4 and 257 <= hidden <= 320) or (inputs == 6 and 449 <= hidden <= 512)
    return supported(inputs, hidden, minibatch) or (wide and minibatch % 32 == 0 and 32 <= minibatch <= 4096)
