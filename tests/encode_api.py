"""sdv_encode_geometry / sdv_encode_frames / sdv_reset_encoder (include/sdvpcm.h) for the tests: the ctypes mirror of the descriptor, `tape_words`
and `tape_frames` - the format as the header's text states it, in numpy, on top of synth.interleave_stream / interleave_stream_f1 / line_bits /
render_lines, which the real reference decodes in the other suites; they never look at the code under test - and `run_call`, one call through a
memory of tests/device_calls.py (HOST: the emulator build, DEVICE: the product on the GPU) with every byte of the destination buffer compared:
the rows, their padding, what lies in front of and behind the stated span."""
import ctypes as C

import numpy as np

import device_calls as dc
from sdvpcmdecoder_amd import abi, synth

NTSC, PAL = abi.ENC_NTSC, abi.ENC_PAL
BIT14, BIT16 = abi.ENC_14BIT, abi.ENC_16BIT
TFF, BFF = abi.ENC_TFF, abi.ENC_BFF
COPY_PROHIBITED, EMPHASIS = abi.ENC_CTRL_COPY_PROHIBITED, abi.ENC_CTRL_EMPHASIS
OK, BAD_ARG, NULL_VIDEO, NULL_PCM = abi.OK, abi.ERR_BAD_ARG, abi.ERR_NULL_VIDEO, abi.ERR_NULL_PCM
LPF = {NTSC: 245, PAL: 294}
FPS = {NTSC: 60, PAL: 50}
FILL, TAIL = 0x5A, 64           # what a destination buffer holds before the call; bytes behind its stated span


Desc = abi.EncodeDesc


def desc(std=NTSC, res=BIT14, ctrl=0, ctrl_flags=0, order=TFF, black=30, white=200, tc=(0, 0, 0, 0, 0), width=720, height=486,
         data_start=12, data_stop=708, top_line=0):
    """tc: (index, hour, minute, second, field)"""
    return Desc(std, res, ctrl, ctrl_flags, order, black, white, 0, tc[0], tc[1], tc[2], tc[3], tc[4], (C.c_uint8 * 3)(), width, height,
                data_start, data_stop, top_line)


bind = abi.bind


def emu(emu_lib):
    """the emulator build through device_calls' handle, with the encode entries bound"""
    return bind(dc.emu_lib_of(emu_lib))


def product():
    return bind(dc.product_lib())


def geometry(lib, d):
    """(rc, pairs a frame consumes, lines per field, bytes of a row)"""
    pairs, lines, rb = C.c_size_t(0), C.c_int(-1), C.c_size_t(0)
    rc = lib.sdv_encode_geometry(C.byref(d), C.byref(pairs), C.byref(lines), C.byref(rb))
    return rc, pairs.value, lines.value, rb.value


def pairs_per_frame(std):
    return 2 * LPF[std] * 3


# ---- the header's text ------------------------------------------------------------------------------------------------------------------------
def time_code(std, tc, field_no):
    """(hour, minute, second, field) of field `field_no` of a tape whose first field has tc = (index, hour, minute, second, field)"""
    fps = FPS[std]
    t = (((tc[1] * 60 + tc[2]) * 60 + tc[3]) * fps + tc[4] + field_no) % (16 * 3600 * fps)
    return t // (3600 * fps), (t // (60 * fps)) % 60, (t // fps) % 60, t % fps


def ctrl_words(std, res, ctrl_flags, tc, field_no):
    """the eight words of the control line of a field"""
    hour, minute, second, field = time_code(std, tc, field_no)
    ctrl = (8 if ctrl_flags & COPY_PROHIBITED else 0) | (2 if res == BIT16 else 0) | (0 if ctrl_flags & EMPHASIS else 1)
    return [0x3333, 0x0CCC, 0x3333, 0x0CCC, 0, tc[0] << 8 | hour << 4 | minute >> 2, (minute & 3) << 12 | second << 6 | field, ctrl]


def tape_words(pcm, n_frames, std=NTSC, res=BIT14, ctrl=0, ctrl_flags=0, tc=(0, 0, 0, 0, 0)):
    """pcm: (n_pairs, 2) int16, the whole tape from its reset -> the lines of its first n_frames frames, (2 n_frames, lines per field, 9) uint16:
    eight words and the CRC.  Pairs the frames do not reach are left out, pairs they lack are silence.  ctrl_flags: one value, or one per frame
    (a tape made in calls whose descriptors differ)."""
    lpf = LPF[std]
    n_blocks = n_frames * 2 * lpf
    samples = np.zeros((n_blocks * 3, 2), dtype=np.int16)
    pcm = np.asarray(pcm, dtype=np.int16).reshape(-1, 2)[:n_blocks * 3]
    samples[:len(pcm)] = pcm
    words16 = samples.view(np.uint16).reshape(n_blocks, 6).astype(np.uint32)         # L0 R0 L1 R1 L2 R2
    w9 = synth.interleave_stream_f1(words16) if res == BIT16 else synth.interleave_stream((words16 >> 2) & 0x3FFF)
    w9 = w9.reshape(2 * n_frames, lpf, 9)
    if not ctrl:
        return w9
    flags = np.broadcast_to(np.asarray(ctrl_flags), (n_frames,))
    cb = np.array([ctrl_words(std, res, int(flags[f // 2]), tc, f) for f in range(2 * n_frames)], dtype=np.uint32)
    cb9 = np.concatenate([cb, synth.crc16_words14(cb)[:, None].astype(np.uint32)], axis=1).astype(np.uint16)
    return np.concatenate([cb9[:, None, :], w9], axis=1)


def tape_frames(w9, d, frames=None):
    """the lines of a tape (tape_words) -> the frames `frames` (a range; default all) by the geometry, levels and field order of descriptor d:
    (n, height, width) uint8.  Row 2 r: line top_line + r of the field first in time (of the other with BFF), row 2 r + 1: the other field's; rows
    without a line and the last row of an odd height are black."""
    n_fields, lpft, _ = w9.shape
    frames = list(range(n_fields // 2) if frames is None else frames)
    out = np.full((len(frames), d.height, d.width), d.black, dtype=np.uint8)
    rows = np.arange(d.height & ~1)
    line = d.top_line + rows // 2
    live = (line >= 0) & (line < lpft)
    if not live.any() or not frames:
        return out
    rows, line = rows[live], line[live]
    field = 2 * np.asarray(frames)[:, None] + ((rows & 1) ^ (1 if d.field_order == BFF else 0))[None, :]
    words = w9[field, line[None, :]].reshape(-1, 9)
    luma = synth.render_lines(synth.line_bits(words), width=d.width, black=d.black, white=d.white, x0=d.data_start, x1=d.data_stop)
    out[:, rows] = luma.reshape(len(frames), len(rows), d.width)
    return out


def cells_of(luma, white):
    """a frame made with width 137 * 4 and the window the whole row -> its cells (..., rows, 137) as 0 / 1; the four pixels of a cell agree"""
    assert luma.shape[-1] == 137 * 4
    q = luma.reshape(luma.shape[:-1] + (137, 4))
    assert (q == q[..., :1]).all()
    return (q[..., 0] == white).astype(np.uint32)


def words_of(cells):
    """cells (..., 137) -> (the eight words and the CRC (..., 9), markers as they should be)"""
    c = np.asarray(cells, dtype=np.uint32)
    ok = (c[..., :4] == [1, 0, 1, 0]).all(axis=-1) & (c[..., 132:] == [0, 1, 1, 1, 1]).all(axis=-1)
    data = c[..., 4:116].reshape(c.shape[:-1] + (8, 14))
    words = (data << np.arange(13, -1, -1, dtype=np.uint32)).sum(axis=-1)
    crc = (c[..., 116:132] << np.arange(15, -1, -1, dtype=np.uint32)).sum(axis=-1)
    return np.concatenate([words, crc[..., None]], axis=-1), ok


# ---- one call ---------------------------------------------------------------------------------------------------------------------------------
def run_call(via, lib, eng, d, pcm, n_pairs, n_frames, want, dst_off=0, dst_pad=0, frame_pad=0, pcm_off=0, expect_rc=OK):
    """One sdv_encode_frames call: `pcm` (n, 2) int16 is uploaded behind pcm_off bytes, n_pairs of its pairs are stated; `want` (n_frames, height,
    width) is what the call has to leave.  Asserts the return code and EVERY byte of the destination buffer."""
    pcm = np.ascontiguousarray(np.asarray(pcm, dtype=np.int16).reshape(-1, 2))
    raw = np.concatenate([np.full(pcm_off, 0xC3, dtype=np.uint8), pcm.view(np.uint8).reshape(-1), np.full(8, 0xC3, dtype=np.uint8)])
    drs = d.width + dst_pad
    dfs = d.height * drs + frame_pad
    span = (n_frames - 1) * dfs + (d.height - 1) * drs + d.width if n_frames > 0 else 0
    expect = np.full(dst_off + span + TAIL, FILL, dtype=np.uint8)
    sbuf, dbuf = via.array(raw), via.array(expect.copy())
    rc = lib.sdv_encode_frames(eng, C.byref(d), via.ptr(sbuf, pcm_off), n_pairs, n_frames, via.ptr(dbuf, dst_off), drs, dfs, via.stream())
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
