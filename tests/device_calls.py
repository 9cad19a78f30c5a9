"""Device-side counterparts of the host-memory call helpers the emulator tests use (engine_api.emu_*, audio_api.emu_audio / emu_run and the
raw calls some tests make themselves): the same arguments and the same return values (numpy arrays, rc, counts), through ctypes on the C-ABI
of the product library with torch device buffers.

A test body is written once against a "memory" - HOST (the emulator build: numpy arrays, the helpers of engine_api / audio_api) or DEVICE (the
product library on the GPU) - and its test_emu_* / test_gpu_* twins hand it one or the other (tests/test_twins.py keeps the pairs together).

Every DEVICE output buffer is allocated with a guard behind the capacity that is stated to the call: the rest of what the call would have
needed had the stated capacity been the usual one, then GUARD records, all filled with a pattern.  `get` and `check` assert that nothing behind
the stated capacity was written, after every call, refused calls included: a kernel that ignores a small capacity fails an assertion and still
writes inside the allocation.

The library is loaded through a handle of its own (as stream_scenarios.bind does), so that the argument types set here and the ones the
package sets on its handle do not meet; engines are made with sdv_engine_create, as the bodies make them on the emulator build.  Calls go to
torch's current stream, the one the buffers are filled and read on (tests/test_stream_contract.py is where side streams are tested)."""
import ctypes as C

import numpy as np

import audio_api as A
import engine_api as ea
from sdvpcmdecoder_amd import abi
from stitch_api import PAIR_DTYPE

GUARD = 256             # records behind every device output buffer
PATTERN = 0xA5


# ---- memory -----------------------------------------------------------------------------------------------------------------------------
class Host:
    """numpy arrays: what the emulator build reads and writes.  dirty: an output buffer starts as PATTERN bytes, not as zeros - a call has to write
    every byte of every record it counts (tests/test_memory_history.py)."""
    name = "host"

    def __init__(self, dirty=False):
        self.dirty = dirty

    def zeros(self, n, dtype, full=None):
        if self.dirty:
            return np.full(int(n) * np.dtype(dtype).itemsize, PATTERN, dtype=np.uint8).view(dtype)
        return np.zeros(n, dtype=dtype)

    def array(self, a):
        return np.ascontiguousarray(a)

    def ptr(self, b, at=0):
        return b.ctypes.data + at * b.dtype.itemsize

    def get(self, b, n=None, at=0):
        return b.reshape(-1)[at:None if n is None else at + n].copy()

    def check(self, *bufs):
        pass

    def stream(self):
        return None


class DevBuf:
    """`n` records of `dtype` on the device, zeroed (dirty: left as PATTERN bytes, like the guard), with the guard behind them."""

    def __init__(self, n, dtype, full=None, data=None, device="cuda:0", dirty=False):
        import torch
        self.dtype, self.n = np.dtype(dtype), int(n)
        self.total = max(self.n, int(full or 0)) + GUARD
        size = self.dtype.itemsize
        self.t = torch.full((self.total * size,), PATTERN, dtype=torch.uint8, device=device)
        if data is not None:
            self.t[:self.n * size] = torch.from_numpy(np.ascontiguousarray(data).view(np.uint8).reshape(-1).copy()).to(device)
        elif not dirty:
            self.t[:self.n * size] = 0

    def __len__(self):
        return self.n

    def check(self):
        tail = self.t[self.n * self.dtype.itemsize:]
        assert int(tail.min()) == PATTERN and int(tail.max()) == PATTERN, \
            "written behind the stated capacity of %d %s records (first at byte %d behind it)" % (
                self.n, self.dtype.names and self.dtype.names[0] or self.dtype, int((tail != PATTERN).nonzero()[0]))

    def get(self, n=None, at=0):
        self.check()
        n = self.n - at if n is None else n
        assert 0 <= at and at + n <= self.n
        size = self.dtype.itemsize
        return self.t[at * size:(at + n) * size].cpu().numpy().view(self.dtype).reshape(-1).copy()


class Device:
    """torch device buffers with guards: what the product library reads and writes.  dirty: as Host's."""
    name = "device"

    def __init__(self, dirty=False):
        self.dirty = dirty

    def zeros(self, n, dtype, full=None):
        return DevBuf(n, dtype, full, dirty=self.dirty)

    def array(self, a):
        a = np.ascontiguousarray(a)
        return DevBuf(a.size, a.dtype, data=a)

    def ptr(self, b, at=0):
        return b.t.data_ptr() + at * b.dtype.itemsize

    def get(self, b, n=None, at=0):
        return b.get(n, at)

    def check(self, *bufs):
        for b in bufs:
            b.check()

    def stream(self):
        import torch
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _in(mem, recs):
    """(buffer or None, address or None) of an input: an empty input goes in as a null pointer, as the host helpers pass it."""
    recs = np.ascontiguousarray(recs)
    if not len(recs):
        return None, None
    b = mem.array(recs)
    return b, mem.ptr(b)


# ---- the calls, written once for both memories ---------------------------------------------------------------------------------------------
class Calls:
    """The helpers of engine_api / audio_api by their names without the `emu_`: HOST's are those helpers themselves, DEVICE's are the methods below."""

    def __init__(self, mem):
        self.mem = mem
        for nm in ("zeros", "array", "ptr", "get", "check", "stream"):
            setattr(self, nm, getattr(mem, nm))
        self.name = mem.name
        self.last_counts = None         # (blocks, sub-lines) of the last pcm1_stitch_vis
        self.last_count = None          # blocks / lines of the last pcm16_stitch_vis / pcm16_stitch_lines

    def _stitch(self, lib, fn, eng, recs, frasm, pair_full, frame_full, pair_cap, frame_cap):
        mem = self.mem
        pair_cap, frame_cap = pair_cap or pair_full, frame_cap or frame_full
        pairs, frames = mem.zeros(pair_cap, PAIR_DTYPE, pair_full), mem.zeros(frame_cap, frasm, frame_full)
        src, addr = _in(mem, recs)
        npairs, nframes = C.c_size_t(0), C.c_size_t(0)
        rc = getattr(lib, fn)(eng, addr, len(recs), mem.ptr(pairs), pair_cap, C.byref(npairs), mem.ptr(frames), frame_cap, C.byref(nframes), mem.stream())
        return rc, mem.get(pairs, min(npairs.value, pair_cap)), mem.get(frames, min(nframes.value, frame_cap))

    def stitch(self, lib, eng, recs, settings=None, pair_cap=None, frame_cap=None):
        """engine_api.emu_stitch"""
        import stitch_api as sa
        if settings is not None:
            assert lib.sdv_set_stitch_settings(eng, C.byref(settings)) == 0
        nfr = int((recs["service_type"] == 5).sum()) + 2
        return self._stitch(lib, "sdv_stitch_frames", eng, recs, sa.FRASM_DTYPE, nfr * 2400 + 16, nfr * 3, pair_cap, frame_cap)

    def pcm1_stitch(self, lib, eng, recs, settings=None, pair_cap=None, frame_cap=None):
        """engine_api.emu_pcm1_stitch"""
        import pcm1_api as p1
        if settings is not None:
            assert lib.sdv_set_pcm1_stitch_settings(eng, C.byref(settings)) == 0
        nfr = int((recs["service_type"] == 5).sum()) + 2
        return self._stitch(lib, "sdv_pcm1_stitch_frames", eng, recs, p1.FRASM1_DTYPE, nfr * 1472 + 16, nfr + 8, pair_cap, frame_cap)

    def pcm16_stitch(self, lib, eng, recs, settings=None, pair_cap=None, frame_cap=None):
        """engine_api.emu_pcm16_stitch"""
        import pcm16_api as p16
        if settings is not None:
            assert lib.sdv_set_pcm16x0_stitch_settings(eng, C.byref(settings)) == 0
        nfr = int((recs["service_type"] == 5).sum()) + 2
        return self._stitch(lib, "sdv_pcm16x0_stitch_frames", eng, recs, p16.FRASM16_DTYPE, nfr * 1472 + 16, nfr + 8, pair_cap, frame_cap)

    def pcm1_stitch_vis(self, lib, eng, recs, settings=None, blocks=True, lines=True, block_cap=None, line_cap=None):
        """engine_api.emu_pcm1_stitch_vis"""
        import pcm1_api as p1
        mem = self.mem
        nfr = int((recs["service_type"] == 5).sum()) + 2
        bl = mem.zeros(block_cap if block_cap is not None else nfr * 16, p1.BLOCK1_DTYPE, nfr * 16)
        ln = mem.zeros(line_cap if line_cap is not None else nfr * 1470, p1.ASM1_DTYPE, nfr * 1470)
        assert lib.sdv_set_pcm1_stitch_block_output(eng, mem.ptr(bl) if blocks else None, len(bl)) == 0
        assert lib.sdv_set_pcm1_stitch_line_output(eng, mem.ptr(ln) if lines else None, len(ln)) == 0
        rc, pairs, frames = self.pcm1_stitch(lib, eng, recs, settings)
        nb, nl = lib.sdv_pcm1_stitch_block_count(eng), lib.sdv_pcm1_stitch_line_count(eng)
        self.last_counts = (nb, nl)          # what the call made (or needed)
        assert lib.sdv_set_pcm1_stitch_block_output(eng, None, 0) == 0 and lib.sdv_set_pcm1_stitch_line_output(eng, None, 0) == 0
        return rc, pairs, frames, mem.get(bl, min(nb, len(bl))), mem.get(ln, min(nl, len(ln)))

    def pcm16_stitch_vis(self, lib, eng, recs, settings=None, block_cap=None):
        """engine_api.emu_pcm16_stitch_vis"""
        import pcm16_api as p16
        mem = self.mem
        nfr = int((recs["service_type"] == 5).sum()) + 2
        bl = mem.zeros(block_cap if block_cap is not None else nfr * 800 + 16, p16.VBLOCK16_DTYPE, nfr * 800 + 16)
        assert lib.sdv_set_pcm16x0_stitch_block_output(eng, mem.ptr(bl), len(bl)) == 0
        rc, pairs, frames = self.pcm16_stitch(lib, eng, recs, settings)
        nb = lib.sdv_pcm16x0_stitch_block_count(eng)
        self.last_count = nb
        assert lib.sdv_set_pcm16x0_stitch_block_output(eng, None, 0) == 0
        return rc, pairs, frames, mem.get(bl, min(nb, len(bl)))

    def pcm16_stitch_lines(self, lib, eng, recs, settings=None, line_cap=None):
        """engine_api.emu_pcm16_stitch_lines"""
        mem = self.mem
        nfr = int((recs["service_type"] == 5).sum()) + 2
        ln = mem.zeros(line_cap if line_cap is not None else nfr * 3000 + 16, recs.dtype, nfr * 3000 + 16)
        assert lib.sdv_set_pcm16x0_stitch_line_output(eng, mem.ptr(ln), len(ln)) == 0
        rc, pairs, frames = self.pcm16_stitch(lib, eng, recs, settings)
        nl = lib.sdv_pcm16x0_stitch_line_count(eng)
        self.last_count = nl
        assert lib.sdv_set_pcm16x0_stitch_line_output(eng, None, 0) == 0
        return rc, pairs, frames, mem.get(ln, min(nl, len(ln)))

    def audio(self, lib, eng, pairs, stop, out_cap=None, purges_cap=None):
        """audio_api.emu_audio: (rc, out, purges, masked, n_out, n_purges)"""
        mem = self.mem
        pairs = np.ascontiguousarray(pairs)
        out_full, pur_full = len(pairs) + 1024, int((pairs["service_type"] != 0).sum()) + 2
        out_cap = out_full if out_cap is None else out_cap
        purges_cap = pur_full if purges_cap is None else purges_cap
        out, pur = mem.zeros(out_cap, PAIR_DTYPE, out_full), mem.zeros(purges_cap, A.PURGE_DTYPE, pur_full)      # (a capacity of 0: the guard alone)
        src, addr = _in(mem, pairs)
        n_out, n_pur, nm = C.c_size_t(0), C.c_size_t(0), C.c_uint64(0)
        rc = lib.sdv_audio_process(eng, addr, len(pairs), stop, mem.ptr(out), out_cap, C.byref(n_out), mem.ptr(pur), purges_cap, C.byref(n_pur), C.byref(nm),
                                   mem.stream())
        return rc, mem.get(out, min(n_out.value, out_cap)), mem.get(pur, min(n_pur.value, purges_cap)), nm.value, n_out.value, n_pur.value

    def run(self, lib, pairs, mode, ends, stop):
        """audio_api.emu_run: the bursts of a case through a fresh engine -> (out, purges, masked)."""
        eng = lib.sdv_engine_create(0)
        assert lib.sdv_set_audio_masking(eng, mode) == 0
        outs, purs, masked, a, got = [], [], 0, 0, 0
        try:
            for k, b in enumerate(ends):
                b = int(b)
                rc, o, p, m, _, _ = self.audio(lib, eng, pairs[a:b], 1 if (stop and k + 1 == len(ends)) else 0)
                assert rc == 0, lib.sdv_last_error(eng)
                p = p.copy()
                p["first_pair"] += got
                p["tag_index"] += a
                outs.append(o.copy()); purs.append(p); masked += m
                got += len(o); a = b
        finally:
            lib.sdv_engine_destroy(eng)
        return np.concatenate(outs), np.concatenate(purs), masked

    def binarize(self, lib, eng, luma, first_frame_no=1, flags=1):
        """engine_api.emu_binarize (contiguous frames): (rc, records, frame stats)"""
        import libs
        mem = self.mem
        n, h, w = luma.shape
        nrec = n * (h + 3) + (1 if flags & 1 else 0) + (h + 4 if flags & 4 else 0)
        recs, stats = mem.zeros(nrec, libs.LINE_DTYPE), mem.zeros(n + (1 if flags & 4 else 0), ea.STATS_DTYPE)
        src = mem.array(luma)
        rc = lib.sdv_binarize_frames(eng, mem.ptr(src), w, w * h, w, h, n, first_frame_no, flags, mem.ptr(recs), len(recs), mem.ptr(stats), len(stats), mem.stream())
        return rc, mem.get(recs), mem.get(stats)

    def frames(self, lib, pf, eng, luma, mode, st, first_frame_no=1, configure=True):
        """pcm1_frames_api / pcm16_frames_api (`pf`) .run_engine: sdv_pcm1_binarize_frames / sdv_pcm16x0_binarize_frames, one call for all frames"""
        import libs
        mem = self.mem
        f = getattr(lib, "sdv_pcm1_binarize_frames" if hasattr(pf, "BIN1_DTYPE") else "sdv_pcm16x0_binarize_frames")
        dtype = pf.BIN1_DTYPE if hasattr(pf, "BIN1_DTYPE") else pf.BIN16_DTYPE
        if configure:
            lib.sdv_set_mode(eng, mode)
            lib.sdv_set_bin_preset(eng, C.byref(pf._preset(st)))
            lib.sdv_set_check_line_dup(eng, st.get("check_line_dup", 1))
        luma = np.ascontiguousarray(luma)
        n, h, w = luma.shape
        recs, stats = mem.zeros(pf.n_records(n, h, st), dtype), mem.zeros(n + (1 if st.get("end_file") else 0), pf.STATS_DTYPE)
        flags = (1 if st.get("new_file") else 0) | (2 if st.get("doubled") else 0) | (4 if st.get("end_file") else 0)
        src = mem.array(luma)
        rc = f(eng, mem.ptr(src), w, w * h, w, h, n, first_frame_no, flags, mem.ptr(recs), len(recs), mem.ptr(stats), len(stats), mem.stream())
        return rc, mem.get(recs), mem.get(stats)

    def render_lines(self, lib, eng, kind, recs, cap=None):
        """sdv_vis_render_lines over `recs` -> (rc, canvases, frames the call counted): test_render._emu_run"""
        import render_api as ra
        mem = self.mem
        w, h = ra.SIZE[kind]
        full = ra.n_frames(recs) if "service_type" in (recs.dtype.names or ()) else (cap or 0)
        n = full if cap is None else cap
        out = mem.zeros(max(n, 1) * h * w, np.uint32, max(full, 1) * h * w)
        got = C.c_size_t(0)
        src, addr = _in(mem, recs)
        rc = lib.sdv_vis_render_lines(eng, kind, addr, len(recs), mem.ptr(out), n, C.byref(got), mem.stream())
        return rc, mem.get(out, min(got.value, n) * h * w).reshape(-1, h, w), got.value

    def render_rows(self, lib, fn, eng, kind, rows, n_rows, per):
        """sdv_vis_render_blocks / sdv_vis_render_asm_lines (`fn`) over the first n_rows records of the buffer `rows`, `per` of them per frame (a host
        array) -> (rc, canvases)"""
        import render_api as ra
        mem = self.mem
        w, h = ra.SIZE[kind]
        per = np.ascontiguousarray(per, dtype=np.uint32)
        out = mem.zeros(max(len(per), 1) * h * w, np.uint32)
        rc = getattr(lib, fn)(eng, kind, mem.ptr(rows), n_rows, per.ctypes.data, len(per), mem.ptr(out), len(per), mem.stream())
        return rc, mem.get(out, len(per) * h * w).reshape(-1, h, w)


class HostCalls(Calls):
    """The emulator build: the helpers of engine_api / audio_api as they are."""

    def __init__(self):
        Calls.__init__(self, Host())
        self.stitch, self.pcm1_stitch, self.pcm16_stitch = ea.emu_stitch, ea.emu_pcm1_stitch, ea.emu_pcm16_stitch
        self.audio, self.run, self.binarize = A.emu_audio, A.emu_run, ea.emu_binarize

    def frames(self, lib, pf, *a, **kw):
        return pf.run_engine(lib, *a, **kw)

    def pcm1_stitch_vis(self, *a, **kw):
        out = ea.emu_pcm1_stitch_vis(*a, **kw)
        self.last_counts = ea.emu_pcm1_stitch_vis.last_counts
        return out

    def pcm16_stitch_vis(self, *a, **kw):
        out = ea.emu_pcm16_stitch_vis(*a, **kw)
        self.last_count = ea.emu_pcm16_stitch_vis.last_count
        return out

    def pcm16_stitch_lines(self, *a, **kw):
        out = ea.emu_pcm16_stitch_lines(*a, **kw)
        self.last_count = ea.emu_pcm16_stitch_lines.last_count
        return out


HOST = HostCalls()
DEVICE = Calls(Device())


# ---- the two libraries behind one set of argument types --------------------------------------------------------------------------------------
bind_all = abi.bind          # every entry point the twinned bodies call, on either build


_product = None


def product_lib():
    """The product library through a handle of this module's own (torch brings up the HIP runtime first, as sdvpcmdecoder_amd.Engine has it)."""
    global _product
    if _product is None:
        import torch
        from sdvpcmdecoder_amd import load_library
        torch.cuda.init()
        _product = bind_all(C.CDLL(load_library()._name))
    return _product


def emu_lib_of(lib):
    """The emulator build through a handle of this module's own."""
    return bind_all(C.CDLL(lib._name))
