"""sdv_encode_markerless_geometry / sdv_encode_markerless_frames (include/sdvpcm.h) for the tests: the ctypes mirror of the descriptor, `tape_bits` and
`tape_frames` - the two formats as the header's text states them, in numpy, on top of synth.pcm1_crc_words / pcm1_line_bits / pcm16x0_encode_fields /
pcm16x0_crc_words / pcm16x0_line_bits / render_lines, which the real reference decodes in the other suites; they never look at the code under test -
and `run_call`, one call through a memory of tests/device_calls.py (HOST: the emulator build, DEVICE: the product on the GPU) with every byte of the
destination buffer compared: the rows, their padding, what lies in front of and behind the stated span."""
import ctypes as C

import numpy as np

import device_calls as dc
from sdvpcmdecoder_amd import abi, synth

PCM1, SI, EI = abi.ENC_FMT_PCM1, abi.ENC_FMT_PCM16X0_SI, abi.ENC_FMT_PCM16X0_EI
TFF, BFF = abi.ENC_TFF, abi.ENC_BFF
EMPHASIS, RATE_44100, CODE = abi.ENC_ML_EMPHASIS, abi.ENC_ML_RATE_44100, abi.ENC_ML_CODE
OK, BAD_ARG, NULL_VIDEO, NULL_PCM = abi.OK, abi.ERR_BAD_ARG, abi.ERR_NULL_VIDEO, abi.ERR_NULL_PCM
CELLS = {PCM1: 94, SI: 193, EI: 193}
PAIRS_PER_FRAME, FIELD_PAIRS, LINES = 1470, 735, 245
HEADER_WORDS = (0x0666, 0x0CCC, 0x1999, 0x1333, 0x0666, 0x0CCC, 0xCCCC)
FILL, TAIL = 0x5A, 64           # what a destination buffer holds before the call; bytes behind its stated span


Desc = abi.EncodeMarkerlessDesc


def desc(fmt=PCM1, order=TFF, black=30, white=200, header=0, ctrl_flags=0, width=720, height=490, data_start=4, data_stop=716, top_line=0):
    return Desc(fmt, order, black, white, header, ctrl_flags, (C.c_uint8 * 2)(), width, height, data_start, data_stop, top_line)


bind = abi.bind


def emu(emu_lib):
    """the emulator build through device_calls' handle, with every entry bound"""
    return bind(dc.emu_lib_of(emu_lib))


def product():
    return bind(dc.product_lib())


def geometry(lib, d):
    """(rc, pairs a frame consumes, lines per field, bytes of a row)"""
    pairs, lines, rb = C.c_size_t(0), C.c_int(-1), C.c_size_t(0)
    rc = lib.sdv_encode_markerless_geometry(C.byref(d), C.byref(pairs), C.byref(lines), C.byref(rb))
    return rc, pairs.value, lines.value, rb.value


# ---- the header's text ------------------------------------------------------------------------------------------------------------------------
def pcm1_word(s):
    """the 13-bit word of 16-bit samples"""
    s = np.asarray(s).astype(np.int64)
    return np.where((s >= -8192) & (s < 8192), 0x1000 | ((s >> 2) & 0x0FFF), (s >> 4) & 0x0FFF).astype(np.uint16)


def pcm1_kept(s):
    """what comes back of 16-bit samples: s & ~3 inside -8192 .. 8191, s & ~15 outside"""
    s = np.asarray(s).astype(np.int64)
    return np.where((s >= -8192) & (s < 8192), s & ~3, s & ~15).astype(np.int16)


def pcm1_sub_line(n):
    """the sub-line of a field that pair n = 0 .. 734 of the field sits on"""
    n = np.asarray(n)
    itl, p = n // 92, n % 92
    wp, even = p >> 1, p & 1
    return 92 * itl + np.where((itl % 2 == 0) == (even == 1), 0, 46) + wp


assert sorted(pcm1_sub_line(np.arange(FIELD_PAIRS)).tolist()) == list(range(FIELD_PAIRS))


def _padded(pcm, n_frames):
    """the pairs n_frames frames take, silence where they lack"""
    out = np.zeros((n_frames * PAIRS_PER_FRAME, 2), dtype=np.int16)
    pcm = np.asarray(pcm, dtype=np.int16).reshape(-1, 2)[:len(out)]
    out[:len(pcm)] = pcm
    return out


def pcm1_words(pcm, n_frames, header=0):
    """pcm: (n_pairs, 2) int16 from the first frame's first pair -> (2 n_frames, header + 245, 7) uint16: the lines of every field, six words and the CRC"""
    words = pcm1_word(_padded(pcm, n_frames)).reshape(2 * n_frames, FIELD_PAIRS, 2)
    sub = np.zeros_like(words)
    sub[:, pcm1_sub_line(np.arange(FIELD_PAIRS))] = words
    w6 = sub.reshape(2 * n_frames * LINES, 6)
    w7 = np.concatenate([w6, synth.pcm1_crc_words(w6)[:, None]], axis=1).reshape(2 * n_frames, LINES, 7)
    head = np.broadcast_to(np.array(HEADER_WORDS, dtype=np.uint16), (2 * n_frames, header, 7))
    return np.concatenate([head, w7], axis=1)


def control_bits(fmt, ctrl_flags):
    """the Control Bit of the 245 lines of a PCM-16x0 field"""
    ctrl = np.ones(LINES, dtype=np.uint8)
    for i in range(7):
        if ctrl_flags & EMPHASIS: ctrl[35 * i + 0] = 0
        if ctrl_flags & RATE_44100: ctrl[35 * i + 1] = 0
        if fmt == EI: ctrl[35 * i + 2] = 0
        if ctrl_flags & CODE: ctrl[35 * i + 3] = 0
    return ctrl


def pcm16_words(pcm, n_frames, fmt):
    """-> (2 n_frames, 245, 3, 4) uint16: the three sub-lines of every line of every field, three words and the CRC"""
    words = synth.pcm16x0_encode_fields(_padded(pcm, n_frames), ei=(fmt == EI))         # [frame][field in playback order][735][3]
    crc = synth.pcm16x0_crc_words(words.reshape(-1, 3)).reshape(n_frames, 2, FIELD_PAIRS)
    return np.concatenate([words, crc[..., None]], axis=3).reshape(2 * n_frames, LINES, 3, 4)


def tape_bits(pcm, n_frames, fmt, header=0, ctrl_flags=0):
    """the cells of the lines of n_frames frames: (2 n_frames, lines per field, CELLS) uint8"""
    if fmt == PCM1:
        w = pcm1_words(pcm, n_frames, header)
        return synth.pcm1_line_bits(w.reshape(-1, 7)).reshape(2 * n_frames, LINES + header, 94)
    w = pcm16_words(pcm, n_frames, fmt)
    ctrl = np.broadcast_to(control_bits(fmt, ctrl_flags), (2 * n_frames, LINES))
    return synth.pcm16x0_line_bits(w.reshape(-1, 3, 4), ctrl.reshape(-1)).reshape(2 * n_frames, LINES, 193)


def frames_of_bits(bits, d, frames=None):
    """the lines of a tape (tape_bits) -> the frames `frames` (a range; default all) by the geometry, levels and field order of descriptor d:
    (n, height, width) uint8.  Row 2 r: line top_line + r of the field first in time (of the other with BFF), row 2 r + 1: the other field's; rows
    without a line and the last row of an odd height are black."""
    n_fields, lpft, cells = bits.shape
    frames = list(range(n_fields // 2) if frames is None else frames)
    out = np.full((len(frames), d.height, d.width), d.black, dtype=np.uint8)
    rows = np.arange(d.height & ~1)
    line = d.top_line + rows // 2
    live = (line >= 0) & (line < lpft)
    if not live.any() or not frames:
        return out
    rows, line = rows[live], line[live]
    field = 2 * np.asarray(frames)[:, None] + ((rows & 1) ^ (1 if d.field_order == BFF else 0))[None, :]
    luma = synth.render_lines(bits[field, line[None, :]].reshape(-1, cells), width=d.width, black=d.black, white=d.white, x0=d.data_start, x1=d.data_stop)
    out[:, rows] = luma.reshape(len(frames), len(rows), d.width)
    return out


def tape_frames(pcm, n_frames, d, frames=None):
    """what n_frames frames of descriptor d made from `pcm` look like"""
    return frames_of_bits(tape_bits(pcm, n_frames, d.format, d.header_lines, d.ctrl_flags), d, frames)


def cells_of(luma, white, cells):
    """a frame made with width cells * 4 and the window the whole row -> its cells (..., rows, cells) as 0 / 1; the four pixels of a cell agree"""
    assert luma.shape[-1] == cells * 4
    q = luma.reshape(luma.shape[:-1] + (cells, 4))
    assert (q == q[..., :1]).all()
    return (q[..., 0] == white).astype(np.uint32)


def bits_value(c):
    """cells (..., n) MSB first -> their value"""
    c = np.asarray(c, dtype=np.uint32)
    return (c << np.arange(c.shape[-1] - 1, -1, -1, dtype=np.uint32)).sum(axis=-1)


def fields_of(rows):
    """(frames, 2 lpft, ...) rows of TFF frames -> (2 frames, lpft, ...) lines of the fields in the order of time"""
    return np.stack([rows[:, 0::2], rows[:, 1::2]], axis=1).reshape((2 * rows.shape[0], rows.shape[1] // 2) + rows.shape[2:])


# ---- one call ---------------------------------------------------------------------------------------------------------------------------------
def run_call(via, lib, eng, d, pcm, n_pairs, n_frames, want, dst_off=0, dst_pad=0, frame_pad=0, pcm_off=0, expect_rc=OK):
    """One sdv_encode_markerless_frames call: `pcm` (n, 2) int16 is uploaded behind pcm_off bytes, n_pairs of its pairs are stated; `want` (n_frames,
    height, width) is what the call has to leave.  Asserts the return code and EVERY byte of the destination buffer."""
    pcm = np.ascontiguousarray(np.asarray(pcm, dtype=np.int16).reshape(-1, 2))
    raw = np.concatenate([np.full(pcm_off, 0xC3, dtype=np.uint8), pcm.view(np.uint8).reshape(-1), np.full(8, 0xC3, dtype=np.uint8)])
    drs = d.width + dst_pad
    dfs = d.height * drs + frame_pad
    span = (n_frames - 1) * dfs + (d.height - 1) * drs + d.width if n_frames > 0 else 0
    expect = np.full(dst_off + span + TAIL, FILL, dtype=np.uint8)
    sbuf, dbuf = via.array(raw), via.array(expect.copy())
    rc = lib.sdv_encode_markerless_frames(eng, C.byref(d), via.ptr(sbuf, pcm_off), n_pairs, n_frames, via.ptr(dbuf, dst_off), drs, dfs, via.stream())
    assert rc == expect_rc, (rc, lib.sdv_last_error(eng))
    got = via.get(dbuf)                 # (DEVICE: also the guard behind the buffer)
    if rc == OK and n_frames > 0:
        expect[dst_off + np.arange(n_frames)[:, None, None] * dfs + np.arange(d.height)[None, :, None] * drs + np.arange(d.width)[None, None, :]] = want
    if not np.array_equal(got, expect):
        bad = np.flatnonzero(got != expect)
        raise AssertionError("%d bytes differ, the first at %d of the destination buffer (rows start at %d, stride %d, %d bytes each, %d rows a frame, frames "
                             "%d apart; %d behind them)" % (len(bad), bad[0], dst_off, drs, d.width, d.height, dfs, TAIL))
    assert np.array_equal(via.get(sbuf), raw)           # the samples are read only
    return got[dst_off:dst_off + span]


def frames_of(buf, d, n_frames, dst_pad=0, frame_pad=0):
    """the frames in what run_call returned"""
    drs = d.width + dst_pad
    dfs = d.height * drs + frame_pad
    return buf[np.arange(n_frames)[:, None, None] * dfs + np.arange(d.height)[None, :, None] * drs + np.arange(d.width)[None, None, :]]
