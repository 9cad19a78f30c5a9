"""ctypes loaders for the test-side libraries: the CPU oracle (oracle/liborc.so) and, when it has
been built in this container, the real reference (oracle/_ref/libsdvref.so)."""
import ctypes as C
import os
import subprocess
import numpy as np

from sdvpcmdecoder_amd.abi import LineRec, LINE_DTYPE, BinState, BinPreset  # noqa: F401  (the records of include/sdvpcm.h, shared with the oracle)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def default_preset() -> BinPreset:
    return BinPreset(160, 28, 10, 7, 240, 5, 6, 4, 2, 0, 1, 1, 1, 0, 0, 0)


def rec_tuple(r: LineRec):
    return tuple(list(getattr(r, n)) if n == "words" else getattr(r, n) for n, _ in LineRec._fields_)


def _bind_bin_api(lib, prefix):
    g = lambda n: getattr(lib, prefix + n)
    g("bin_new").restype = C.c_void_p
    g("bin_free").argtypes = [C.c_void_p]
    g("bin_set_mode").argtypes = [C.c_void_p, C.c_int]
    g("bin_set_coord_search").argtypes = [C.c_void_p, C.c_int]
    g("bin_set_preset").argtypes = [C.c_void_p, C.POINTER(BinPreset)]
    g("bin_reset_good").argtypes = [C.c_void_p]
    g("bin_set_good_from_last").argtypes = [C.c_void_p]
    g("bin_set_state").argtypes = [C.c_void_p, C.POINTER(BinState)]
    g("bin_process").argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_uint16, C.c_int, C.c_int,
                                 C.c_int, C.POINTER(LineRec)]
    g("bin_process").restype = C.c_int
    g("crc_stc007").argtypes = [C.POINTER(C.c_uint16)]
    g("crc_stc007").restype = C.c_uint16


class BinApi:
    """Uniform wrapper over the per-line binarizer entry points of either library."""

    def __init__(self, lib, prefix):
        self.lib, self.p = lib, prefix
        self.h = getattr(lib, prefix + "bin_new")()

    def __getattr__(self, name):
        f = getattr(self.lib, self.p + "bin_" + name)
        return lambda *a: f(self.h, *a)

    def process_px(self, px, frame=0, line=1, service=0, doubled=0, empty=0):
        rec = LineRec()
        if px is None:
            ret = getattr(self.lib, self.p + "bin_process")(self.h, None, 0, frame, line, service, doubled, empty, C.byref(rec))
        else:
            px = np.ascontiguousarray(px, dtype=np.uint8)
            ret = getattr(self.lib, self.p + "bin_process")(self.h, px.ctypes.data, px.shape[0], frame, line, service,
                                                           doubled, empty, C.byref(rec))
        return ret, rec

    def close(self):
        getattr(self.lib, self.p + "bin_free")(self.h)


_orc = None
_ref = None


def build_oracle():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle")])


def load_oracle():
    global _orc
    if _orc is None:
        path = os.path.join(ROOT, "oracle", "liborc.so")
        if not os.path.exists(path):
            build_oracle()
        _orc = C.CDLL(path)
        _bind_bin_api(_orc, "orc_")
    return _orc


def ref_available() -> bool:
    return os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libsdvref.so"))


def load_ref():
    """The reference build links the image's Qt (/opt/conda/lib); preload the system libstdc++ first so the
    older one next to Qt is not picked up."""
    global _ref
    if _ref is None:
        for cand in ("/usr/lib/x86_64-linux-gnu/libstdc++.so.6",):
            if os.path.exists(cand):
                C.CDLL(cand, mode=C.RTLD_GLOBAL)
        _ref = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libsdvref.so"))
        _bind_bin_api(_ref, "ref_")
    return _ref
