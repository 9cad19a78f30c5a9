"""What tests/test_pcm_preemphasis.py and tests/test_pcm_resample.py share: the C-ABI of sdv_pcm_preemphasis / sdv_pcm_resample (include/sdvpcm.h),
the two ways to the code under test - the emulator build on host memory, the product library on device memory - and the condition both files hold
an output to.  Buffers are (pairs, 2) int16, interleaved L R."""
import ctypes as C

import numpy as np

from sdvpcmdecoder_amd import abi

OK, BAD_ARG, NULL_LINES, NULL_BLOCK = abi.OK, abi.ERR_BAD_ARG, abi.ERR_NULL_LINES, abi.ERR_NULL_BLOCK


bind = abi.bind


class Emu:
    """The emulator build: host memory."""
    def __init__(self, lib):
        self.lib = bind(lib)
        self.h = C.c_void_p(self.lib.sdv_engine_create(0))

    def close(self):
        self.lib.sdv_engine_destroy(self.h)

    def buffer(self, data):
        """a buffer that holds `data` (any dtype), 16-byte aligned"""
        raw = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        store = np.zeros(raw.size + 16, dtype=np.uint8)
        off = (-store.ctypes.data) % 16
        b = store[off:off + raw.size]
        b[:] = raw
        return b

    def ptr(self, buf, byte_off=0):
        return buf.ctypes.data + byte_off

    def stream(self):
        return None

    def read(self, buf):
        return buf.copy()


class Gpu:
    """The product library: device memory, the engine's C-ABI handle."""
    def __init__(self):
        from sdvpcmdecoder_amd import Engine
        self.eng = Engine(0)
        self.lib, self.h = bind(self.eng.lib), self.eng._h

    def close(self):
        self.eng.close()

    def buffer(self, data):
        import torch
        raw = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        return torch.from_numpy(raw.copy()).to("cuda:0")

    def ptr(self, buf, byte_off=0):
        return buf.data_ptr() + byte_off

    def stream(self):
        import torch
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def read(self, buf):
        return buf.cpu().numpy().copy()


def pcm_of(raw, n_pairs, byte_off=0):
    """n_pairs pairs of a buffer's bytes (Emu.read / Gpu.read) from byte_off on -> (n_pairs, 2) int16"""
    return np.frombuffer(raw.tobytes()[byte_off:byte_off + 4 * n_pairs], dtype="<i2").reshape(-1, 2).copy()


def check(got, want):
    """The condition of both stages (the derivation: the docstrings of the two test files): every word within 1 LSB of the float64 walk, at most 2
    words of a case differ at all, a case holds at most 200 000 samples.  -> the number of words that differ"""
    assert got.shape == want.shape, (got.shape, want.shape)
    d = np.abs(got.astype(np.int64) - want.astype(np.int64))
    differ = int((d != 0).sum())
    print("samples that differ: %d of %d, largest difference %d" % (differ, d.size, int(d.max()) if d.size else 0))
    assert d.size <= 200_000
    assert (d <= 1).all() and differ <= 2, (differ, int(d.max()))
    return differ


def pairs_of(pcm, rate, emphasis=0):
    """(n, 2) int16 -> sdv_sample_pair records at `rate` (what the decode side's stages take)"""
    from stitch_api import PAIR_DTYPE
    a = np.zeros(len(pcm), dtype=PAIR_DTYPE)
    a["audio_word"] = pcm
    a["sample_flags"] = 3           # block ok, word valid
    a["sample_rate"] = rate
    a["emphasis"] = emphasis
    return a
