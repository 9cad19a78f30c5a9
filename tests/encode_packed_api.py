"""out_fmt of sdv_encode_frames / sdv_encode_markerless_frames (include/sdvpcm.h) for the tests: `pack_ref`, the packings as the header's text states
them, in numpy - neutral chroma, an opaque fourth byte, `black` behind the width; it never looks at the code under test - `row_bytes`, and
`run_call`, one call of either encoder through a memory of tests/device_calls.py (HOST: the emulator build, DEVICE: the product on the GPU) with
every byte of the destination buffer compared: the rows, their padding, what lies in front of and behind the stated span.  The planes that go
into pack_ref come from encode_api / encode_markerless_api."""
import ctypes as C

import numpy as np

import encode_api as en
import encode_markerless_api as ml
from sdvpcmdecoder_amd import abi

FORMATS = abi.PIX_FORMATS
GRAY8, UYVY422, YUYV422, V210, GRAY10LE = abi.PIX_GRAY8, abi.PIX_UYVY422, abi.PIX_YUYV422, abi.PIX_V210, abi.PIX_GRAY10LE
RGB24, BGR24, RGB0, BGR0 = abi.PIX_RGB24, abi.PIX_BGR24, abi.PIX_RGB0, abi.PIX_BGR0
PACKED = {n: v for n, v in sorted(FORMATS.items(), key=lambda kv: kv[1]) if v != GRAY8}         # the eight formats of the feature, by name
OK, BAD_ARG = abi.OK, abi.ERR_BAD_ARG
FILL, TAIL = en.FILL, en.TAIL


def row_bytes(fmt, w):
    """the table of the header"""
    if fmt == GRAY8:
        return w
    if fmt in (UYVY422, YUYV422):
        return 4 * ((w + 1) // 2)
    if fmt == V210:
        return 16 * ((w + 5) // 6)
    if fmt == GRAY10LE:
        return 2 * w
    return (3 if fmt in (RGB24, BGR24) else 4) * w


def pack_ref(plane, fmt, black):
    """plane (..., w) uint8, the luma values of rows -> (..., row_bytes) uint8: the packing of the header's table"""
    plane = np.ascontiguousarray(plane, dtype=np.uint8)
    lead, w = plane.shape[:-1], plane.shape[-1]
    if fmt == GRAY8:
        return plane.copy()
    if fmt in (UYVY422, YUYV422):                   # per pixel pair 128 y 128 y / y 128 y 128; the second half of the last pair of an odd w is black
        y = np.full(lead + (2 * ((w + 1) // 2),), black, dtype=np.uint8)
        y[..., :w] = plane
        out = np.full(lead + (2 * y.shape[-1],), 128, dtype=np.uint8)
        out[..., (1 if fmt == UYVY422 else 0)::2] = y
        return out
    if fmt == V210:                                 # component c of a group at bits 10 (c % 3) of word c / 3; luma j is component 2 j + 1, y << 2; chroma 512
        groups = (w + 5) // 6
        y = np.full(lead + (6 * groups,), black, dtype=np.uint32)
        y[..., :w] = plane
        comps = np.full(lead + (groups, 12), 512, dtype=np.uint32)
        comps[..., 1::2] = (y << 2).reshape(lead + (groups, 6))
        c = comps.reshape(lead + (groups, 4, 3))
        words = c[..., 0] | c[..., 1] << 10 | c[..., 2] << 20
        assert not (words >> 30).any()
        return np.ascontiguousarray(words.astype("<u4")).view(np.uint8).reshape(lead + (16 * groups,))
    if fmt == GRAY10LE:
        return np.ascontiguousarray((plane.astype(np.uint16) << 2).astype("<u2")).view(np.uint8).reshape(lead + (2 * w,))
    if fmt in (RGB24, BGR24):
        return np.repeat(plane, 3, axis=-1)
    out = np.full(lead + (w, 4), 255, dtype=np.uint8)                       # y y y 255
    out[..., :3] = plane[..., None]
    return out.reshape(lead + (4 * w,))


def with_fmt(d, fmt, reserved=0, at=1):
    """descriptor d (either encoder's) with out_fmt[0] = fmt and the reserved element out_fmt[at] = reserved -> d"""
    assert at >= 1
    d.out_fmt[0] = fmt
    d.out_fmt[at] = reserved
    return d


def frames_call(lib, d):
    return lib.sdv_encode_frames if isinstance(d, abi.EncodeDesc) else lib.sdv_encode_markerless_frames


def geometry(lib, d):
    """(rc, pairs a frame consumes, lines per field, bytes of a row) by the geometry call of d's encoder"""
    return en.geometry(lib, d) if isinstance(d, abi.EncodeDesc) else ml.geometry(lib, d)


def run_call(via, lib, eng, d, pcm, n_pairs, n_frames, want, dst_off=0, dst_pad=0, frame_pad=0, pcm_off=0, expect_rc=OK, drs=None, dfs=None):
    """One sdv_encode_frames or sdv_encode_markerless_frames call (by the type of d, whose out_fmt is set): `pcm` (n, 2) int16 is uploaded behind
    pcm_off bytes, n_pairs of its pairs are stated; `want` (n_frames, height, width) are the luma PLANES the GRAY8 call has to leave - what this call has
    to leave is pack_ref of them.  drs / dfs: strides other than row_bytes + dst_pad and height * stride + frame_pad (for a refusal).  Asserts the
    return code and EVERY byte of the destination buffer; -> the bytes of the stated span."""
    fmt = int(d.out_fmt[0])
    rb = row_bytes(fmt, d.width)
    pcm = np.ascontiguousarray(np.asarray(pcm, dtype=np.int16).reshape(-1, 2))
    raw = np.concatenate([np.full(pcm_off, 0xC3, dtype=np.uint8), pcm.view(np.uint8).reshape(-1), np.full(8, 0xC3, dtype=np.uint8)])
    rs = rb + dst_pad
    fs = d.height * rs + frame_pad
    span = (n_frames - 1) * fs + (d.height - 1) * rs + rb if n_frames > 0 else 0
    expect = np.full(dst_off + span + TAIL, FILL, dtype=np.uint8)
    sbuf, dbuf = via.array(raw), via.array(expect.copy())
    rc = frames_call(lib, d)(eng, C.byref(d), via.ptr(sbuf, pcm_off), n_pairs, n_frames, via.ptr(dbuf, dst_off), rs if drs is None else drs,
                             fs if dfs is None else dfs, via.stream())
    assert rc == expect_rc, (rc, lib.sdv_last_error(eng))
    got = via.get(dbuf)                 # (DEVICE: also the guard behind the buffer)
    if rc == OK and n_frames > 0:
        packed = pack_ref(want, fmt, d.black)
        assert packed.shape == (n_frames, d.height, rb)
        expect[dst_off + np.arange(n_frames)[:, None, None] * fs + np.arange(d.height)[None, :, None] * rs + np.arange(rb)[None, None, :]] = packed
    if not np.array_equal(got, expect):
        bad = np.flatnonzero(got != expect)
        raise AssertionError("%d bytes differ, the first at %d of the destination buffer (rows start at %d, stride %d, %d bytes each, %d rows a frame, frames "
                             "%d apart; %d behind them): got %d, expected %d" % (len(bad), bad[0], dst_off, rs, rb, d.height, fs, TAIL, got[bad[0]], expect[bad[0]]))
    assert np.array_equal(via.get(sbuf), raw)           # the samples are read only
    return got[dst_off:dst_off + span]


def rows_of(buf, rb, height, n_frames, dst_pad=0, frame_pad=0):
    """the rows in what run_call returned: (n_frames, height, rb)"""
    rs = rb + dst_pad
    fs = height * rs + frame_pad
    return buf[np.arange(n_frames)[:, None, None] * fs + np.arange(height)[None, :, None] * rs + np.arange(rb)[None, None, :]]
