"""Strides and offsets beyond 31 and 32 bits for every entry that takes video at `base + f * frame_stride + r * row_stride` (include/sdvpcm.h): the
case tables, the sparse layout that makes such buffers affordable, and the arithmetic that says which cases can tell a 32-bit offset from a 64-bit one.
Shared by the emulator and the GPU twins of tests/test_far_offsets.py.

The sparse layout.  Only the bytes of the rows are ever written.  On host memory the buffer is np.empty - pages nobody touches cost nothing, a case of
6 GiB takes a few MiB - and on the device one torch allocation filled with FILL, the rows copied in one by one.  No host buffer exceeds HOST_CAP, no
device allocation DEVICE_CAP, and a test holds one such allocation at a time (Sparse.release).

The lead-in.  A wrong kernel has to fail an assertion, not fault.  An offset cut to 32 bits is smaller than the true one and stays inside the
allocation by itself.  An offset that is sign-extended from 32 bits lands up to 2^31 bytes in front of the base, so wherever a case has an offset at
or above 2^31 the base lies LEAD = 2^31 bytes behind the start of the allocation.

Writers.  After the call everything but the destination rows still holds FILL: on the device the whole allocation is scanned, on host memory the
windows where each row would land with its offset cut to 32 bits or sign-extended from 32 bits (filled before the call), and 64 bytes on either side
of every row."""
import functools

import numpy as np

import geometry_cases as gc
from sdvpcmdecoder_amd import synth

FILL = 0x5A
HOST_CAP = 9 << 30                  # bytes of address space of one host buffer
DEVICE_CAP = 17 << 29               # 8.5 GiB: one device allocation
LEAD = 1 << 31
SMALL_LEAD = 4096
EDGE = 64                           # bytes on either side of a row, and behind the last one, that a writer must leave alone
M32 = (1 << 32) - 1

FAR_FRAME_STRIDE = (1 << 31) + 4096         # A: three frames, the second beyond 2 GiB, the third beyond 4 GiB
WRITER_FRAME_STRIDE = 1 << 32               # A, writers: the largest stride they take
WRITER_ROW_STRIDE = (1 << 30) + 16          # B, writers: five rows, rows 2 and 4 at 2^31 + 32 and 2^32 + 64
WRITER_ROWS = 5
ROW_PAD = 16                                # A: row_stride = width + 16


def cut32(o):
    return o & M32


def sign32(o):
    o &= M32
    return o - (1 << 32) if o & (1 << 31) else o


# ---- the layout ---------------------------------------------------------------------------------------------------------------------------------
class Sparse:
    """`n` frames of `h` rows of `w` bytes: row r of frame f at address + f * frame_stride + r * row_stride, in host memory (device=False) or in one
    device allocation.  put() writes rows, rows() reads them back, rest_untouched() says whether anything else was written (see the module's text)."""

    def __init__(self, device, n, h, w, row_stride, frame_stride, align_shift=0):
        self.device, self.n, self.h, self.w, self.row_stride, self.frame_stride = device, n, h, w, row_stride, frame_stride
        assert row_stride >= w and (n == 1 or frame_stride >= (h - 1) * row_stride + w)
        self.offsets = [f * frame_stride + r * row_stride for f in range(n) for r in range(h)]
        far = max(self.offsets) + w
        self.lead = (LEAD if far > (1 << 31) else SMALL_LEAD) + align_shift
        self.total = self.lead + far + EDGE
        assert self.total <= (DEVICE_CAP if device else HOST_CAP), "the case is larger than the suite allows: %d bytes" % self.total
        if device:
            import torch
            self.torch = torch
            self.t = torch.full((self.total,), FILL, dtype=torch.uint8, device="cuda:0")
            assert self.t.data_ptr() % 16 == 0
            self.address = self.t.data_ptr() + self.lead
        else:
            raw = np.empty(self.total + 15, dtype=np.uint8)
            a = (-raw.ctypes.data) % 16
            self.buf = raw[a:a + self.total]
            self.address = self.buf.ctypes.data + self.lead
            self.windows = self._windows()
            for lo, hi in self.windows:
                self.buf[lo:hi] = FILL

    def _windows(self):
        """[lo, hi) in the buffer: around every row, and where a row lands with its offset cut to 32 bits or sign-extended from them"""
        out = []
        for o in self.offsets:
            for at, edge in ((o, EDGE), (cut32(o), 0), (sign32(o), 0)):
                lo, hi = max(0, self.lead + at - edge), min(self.total, self.lead + at + self.w + edge)
                if lo < hi:
                    out.append((lo, hi))
        return sorted(set(out))

    def put(self, frames):
        frames = np.ascontiguousarray(frames).reshape(self.n * self.h, self.w)
        if self.device:
            src = self.torch.from_numpy(frames.copy()).to("cuda:0")          # (a copy: the cases are read-only arrays)
        for i, o in enumerate(self.offsets):
            at = self.lead + o
            if self.device:
                self.t[at:at + self.w] = src[i]
            else:
                self.buf[at:at + self.w] = frames[i]
        return self

    def rows(self):
        """-> (n, h, w), what the rows hold now"""
        if self.device:
            got = self.torch.stack([self.t[self.lead + o:self.lead + o + self.w] for o in self.offsets]).cpu().numpy()
        else:
            got = np.stack([self.buf[self.lead + o:self.lead + o + self.w] for o in self.offsets])
        return got.reshape(self.n, self.h, self.w)

    def rest_untouched(self):
        """True when everything outside the rows still holds FILL.  The rows themselves are given FILL again on the way: call rows() first."""
        for o in self.offsets:
            at = self.lead + o
            (self.t if self.device else self.buf)[at:at + self.w] = FILL
        if self.device:
            lo = hi = None
            for chunk in self.t.split(1 << 30):
                a, b = chunk.min(), chunk.max()
                lo, hi = (a, b) if lo is None else (self.torch.minimum(lo, a), self.torch.maximum(hi, b))
            return int(lo) == FILL and int(hi) == FILL
        return all(bool((self.buf[a:b] == FILL).all()) for a, b in self.windows)

    def release(self):
        if self.device:
            self.t = None
            self.torch.cuda.empty_cache()
        else:
            self.buf = None


def sparse_frames(device, frames, row_stride, frame_stride=None, align_shift=0):
    n, h, w = frames.shape
    fs = frame_stride if frame_stride is not None else h * row_stride
    return Sparse(device, n, h, w, row_stride, fs, align_shift).put(frames)


# ---- which row-term cases can tell --------------------------------------------------------------------------------------------------------------
def aliases(row_stride, height, run, starts=(0, 1, 2)):
    """A run of the capture loops starts at some line s of a field, at a 64-bit address, and reaches line s + j at s's address + j * 2 * row_stride
    formed in 32 bits.  A cut offset that lands between lines gives a CRC failure: the run ends, the line is decoded again line by line, at its true
    address - the defect heals itself.  It shows only where the cut offset of line s + j is the true offset of another line s + j' of the run: then a
    line that reads is recorded in the wrong place.  -> [(field, s, j, j')] for the lines s of `starts` in each field, j' < j < run.  (batch1 and batch16
    begin behind the first line or two of a field, which are taken one by one: s = 0, 1, 2.  The whole-frame capture of STC-007 begins at the frame's
    first row pair and forms every offset from there: s = 0.)"""
    out = []
    for field in (0, 1):
        nl = (height + 1 - field) // 2
        for s in starts:
            reach = min(run, nl - s)
            true = {j * 2 * row_stride: j for j in range(max(reach, 0))}
            for j in range(max(reach, 0)):
                o = j * 2 * row_stride
                if cut32(o) != o and cut32(o) in true:
                    out.append((field, s, j, true[cut32(o)]))
    return out


def can_tell(row_stride, height, run, starts=(0, 1, 2)):
    """Every start of both fields has a line whose cut offset is another line's true one."""
    got = {(field, s) for field, s, _j, _k in aliases(row_stride, height, run, starts)}
    return all((field, s) in got for field in (0, 1) for s in starts)


PCM1_RUN = 64                       # batch1 (pcm1_frames_device.h): lines of a run
PCM16X0_RUN = 21                    # BATCH16_LINES (pcm16_frames_device.h)
STC007_RUN = 1 << 15                # the whole-frame capture (stc007_device.h): a field

# B, the marker-less formats: (generator arguments, mode, row_stride, the longest run)
ROW_CASES = {
    "pcm1": (dict(height=72, seed=401), 2, 1 << 26, PCM1_RUN),                  # 4.5 GiB
    "pcm16x0": (dict(height=24, seed=701), 2, 1 << 28, PCM16X0_RUN),            # 6 GiB
}
# B, STC-007: both sides of the guard of the whole-frame capture (row_stride * height < 2^31) and one case whose rows lie beyond 2^32.
# (height, row_stride, the capture is taken, offsets leave 32 bits)
STC_ROW_CASES = {
    "capture_taken": (64, (1 << 25) - 16, True, False),
    "capture_not_taken": (64, 1 << 25, False, False),
    "rows_beyond_4g": (66, 1 << 26, False, True),
}


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _markerless(fmt_name, n, height, seed):
    fmt = gc.FORMATS[fmt_name]
    return np.ascontiguousarray(fmt.gen_frames(n, height=height, seed=seed)[0])


@functools.lru_cache(maxsize=None)
def row_case(fmt_name):
    """-> (the frame (1, h, w), the oracle's records, its frame descriptors) of ROW_CASES"""
    kw, mode, _rs, _run = ROW_CASES[fmt_name]
    frames = _markerless(fmt_name, 1, **kw)
    recs, stats = gc.FORMATS[fmt_name].frames_api.run_cpu(gc.libs.load_oracle(), "orc_", frames, mode, {})
    return _frozen(frames, recs, stats)


@functools.lru_cache(maxsize=None)
def row_lines_case(fmt_name):
    """The rows of ROW_CASES as lines of their own, nothing preset -> (rows (h, w), the oracle's records, scan_done marks or None)"""
    fmt = gc.FORMATS[fmt_name]
    rows = row_case(fmt_name)[0][0]
    recs, scans = gc._oracle_lines(fmt, rows, gc.cold_states(fmt.recs_per_line * len(rows)), ROW_CASES[fmt_name][1])
    return _frozen(rows, recs) + (scans,)


@functools.lru_cache(maxsize=None)
def frame_case(fmt_name):
    """A: three frames of 720 x 32 -> (frames, the oracle's records, its frame descriptors), MODE_NORMAL"""
    frames = gc.make_frames(gc.FORMATS[fmt_name], 720, 32, n=3, seed=1201)
    recs, stats = gc.FORMATS[fmt_name].frames_api.run_cpu(gc.libs.load_oracle(), "orc_", frames, 2, {})
    return _frozen(frames, recs, stats)


def _stc_oracle(luma):
    from oracle_run import oracle_binarize
    recs, stats = oracle_binarize(luma, mode=2, first_frame_no=1, new_file=True)
    return recs, np.ascontiguousarray(stats).reshape(-1).view(gc.ea.STATS_DTYPE)


@functools.lru_cache(maxsize=None)
def stc_frame_case(tape):
    """A: four STC-007 frames of 720 x 48; the first is decoded from an ordinary buffer (the cold frame: it warms the stream), the other three in one
    call from frames far apart.  "clean": a tape that plays - the lean kernel alone.  "worn" (kernel_path_tapes.unreadable_cells): an unreadable cell
    on every 13th line of those three - the lean kernel gives them up, the general kernel asks for sweeps of the reference level, the sweep kernels
    settle them (they form a line's address from frame and row again, stc007_sweep_device.h), and the rounds behind go to the five-wave kernel.
    -> (luma (4, h, 720), the oracle's records, of which the first `split` belong to the first call, descriptors, split)"""
    from kernel_path_tapes import unreadable_cells
    luma = synth.stc007_frames(4, seed=1214, height=48, noise_sigma=3.0)[0].copy()
    if tape == "worn":
        luma[1:] = unreadable_cells(luma[1:], every=13, seed=29)
    luma = np.ascontiguousarray(luma)
    return _frozen(luma, *_stc_oracle(luma)) + (1 + 48 + 3,)


@functools.lru_cache(maxsize=None)
def stc_row_case(height):
    """B: two frames of a tape that plays; the first is decoded from an ordinary buffer (it is the cold frame and warms the stream), the second from
    the sparse layout.  -> (luma (2, h, 720), the oracle's records of both frames, of which the first `split` belong to the first call, descriptors)"""
    luma = np.ascontiguousarray(synth.stc007_frames(2, seed=1230 + height, height=height, noise_sigma=3.0)[0])
    recs, stats = _stc_oracle(luma)
    return _frozen(luma, recs, stats) + (1 + height + 3,)


@functools.lru_cache(maxsize=None)
def stc_lines_case():
    """The rows of the second frame of stc_row_case(66) as lines of their own, nothing preset -> (rows, the oracle's records)"""
    from test_stc_lines import _oracle_lines
    rows = np.ascontiguousarray(stc_row_case(66)[0][1])
    return _frozen(rows, _oracle_lines(rows, None, 2, first_line=1, line_step=1, frame=1))


@functools.lru_cache(maxsize=None)
def chain_case(pcm_type, which):
    """sdv_decode_frames(NEW_FILE | END_FILE).  "frames": the three frames of geometry_cases.fused_case; "rows": the PCM-1 frame of ROW_CASES.
    -> (frames, pairs, frame descriptors, frame statistics as rows of 32 bytes) from the oracle's two workers"""
    if which == "frames":
        return gc.fused_case(pcm_type)
    assert pcm_type == gc.PCM1
    from test_pcm1 import bin_to_line_recs
    orc = gc.libs.load_oracle()
    frames = row_case("pcm1")[0]
    recs, stats = gc.p1f.run_cpu(orc, "orc_", frames, 2, dict(new_file=True, end_file=True))
    pairs, fr = gc.p1.run_cpu(orc, "orc_", bin_to_line_recs(recs), gc.p1.default_settings())
    return _frozen(frames, pairs, fr, np.ascontiguousarray(stats).view(np.uint8).reshape(-1, 32))


# ---- the writers ----------------------------------------------------------------------------------------------------------------------------------
WRITER_WIDTH = 200
# name -> (encoder, its format, out_fmt): both encoders as GRAY8 and in one packed format each
ENCODERS = {"stc007": ("stc007", 0, "gray8"), "stc007_uyvy422": ("stc007", 0, "uyvy422"), "pcm1": ("markerless", "PCM1", "gray8"),
            "pcm16x0_v210": ("markerless", "SI", "v210")}


def writer_geometry(term, row_bytes):
    """-> (n frames, rows, row_stride, frame_stride): "frames": two frames exactly 2^32 apart, the largest frame_stride the writers take, rows
    ROW_PAD bytes longer than they need be; "rows": one frame of five rows 2^30 + 16 apart, rows 2 and 4 beyond 2^31 and 2^32 (frame_stride is
    not looked at for one frame and strides above 4 GiB are refused: 0)"""
    if term == "frames":
        return 2, 6, row_bytes + ROW_PAD, WRITER_FRAME_STRIDE
    return 1, WRITER_ROWS, WRITER_ROW_STRIDE, 0


@functools.lru_cache(maxsize=None)
def encoder_case(name, n, h):
    """-> (descriptor, pcm (pairs, 2) int16, the packed rows (n, h, row bytes) the call has to leave): the references of encode_api /
    encode_markerless_api (the header's text in numpy) through encode_packed_api.pack_ref"""
    import encode_api as en
    import encode_markerless_api as ml
    import encode_packed_api as ep
    which, fmt, out_fmt = ENCODERS[name]
    rng = np.random.default_rng(sum(name.encode()) + n)
    if which == "stc007":
        d = en.desc(width=WRITER_WIDTH, height=h, data_start=2, data_stop=WRITER_WIDTH - 2, top_line=1)
        pcm = rng.integers(-32768, 32768, size=(n * en.pairs_per_frame(en.NTSC), 2), dtype=np.int16)
        planes = en.tape_frames(en.tape_words(pcm, n), d)
    else:
        d = ml.desc(fmt=getattr(ml, fmt), width=WRITER_WIDTH, height=h, data_start=2, data_stop=WRITER_WIDTH - 2, top_line=1)
        pcm = rng.integers(-32768, 32768, size=(n * ml.PAIRS_PER_FRAME, 2), dtype=np.int16)
        planes = ml.tape_frames(pcm, n, d)
    ep.with_fmt(d, ep.FORMATS[out_fmt])
    rows = ep.pack_ref(planes, ep.FORMATS[out_fmt], d.black)
    assert rows.shape[:2] == (n, h) and len({r.tobytes() for r in rows.reshape(n * h, -1)}) == n * h, "every row differs from every other"
    return (d,) + _frozen(pcm, rows)


@functools.lru_cache(maxsize=None)
def ingest_case(n, h):
    """UYVY422 rows of WRITER_WIDTH pixels -> (source rows (n, h, row bytes), the luma ingest_api.ingest_ref makes of them (n, h, width))"""
    import ingest_api as ia
    rng = np.random.default_rng(77 + n)
    luma = rng.integers(0, 256, size=(n, h, WRITER_WIDTH), dtype=np.uint8)
    rows = ia.pack(ia.UYVY422, luma, rng)
    rb = rows.shape[2]
    want, doubled = ia.ingest_ref(rows.reshape(-1), ia.UYVY422, WRITER_WIDTH, h, n, rb, h * rb)
    assert not doubled and np.array_equal(want, luma)
    return _frozen(rows, want)
