"""sdv_ingest_geometry / sdv_ingest_frames (include/sdvpcm.h) for the tests: the ctypes mirror of the descriptor, `ingest_ref` - the contract of
the header comment in numpy (slicing, shifts, np.repeat; it never looks at the code under test or at the oracle) - packers that hide a luma
plane in a packed format, and `run_case`, one call through a memory of tests/device_calls.py (HOST: the emulator build, DEVICE: the product
on the GPU) with every byte of the destination buffer compared: the rows, their padding, what lies in front of and behind the stated span."""
import ctypes as C

import numpy as np

import device_calls as dc
from sdvpcmdecoder_amd import abi

FORMATS = abi.PIX_FORMATS
GRAY8, UYVY422, YUYV422, V210, GRAY10LE = abi.PIX_GRAY8, abi.PIX_UYVY422, abi.PIX_YUYV422, abi.PIX_V210, abi.PIX_GRAY10LE
RGB24, BGR24, RGB0, BGR0 = abi.PIX_RGB24, abi.PIX_BGR24, abi.PIX_RGB0, abi.PIX_BGR0
RGB_FORMATS = (RGB24, BGR24, RGB0, BGR0)
BW, R, G, B = abi.COLOR_BW, abi.COLOR_R, abi.COLOR_G, abi.COLOR_B
OFF, ON, AUTO = abi.INGEST_DOUBLE_OFF, abi.INGEST_DOUBLE_ON, abi.INGEST_DOUBLE_AUTO
OK, BAD_ARG, UNSUPPORTED, NULL_VIDEO, NULL_PCM = abi.OK, abi.ERR_BAD_ARG, abi.ERR_UNSUPPORTED, abi.ERR_NULL_VIDEO, abi.ERR_NULL_PCM
MAX_LINES = 640                 # LINES_PER_FRAME_MAX
FILL, TAIL = 0x5A, 64           # what a destination buffer holds before the call; bytes behind its stated span


Desc = abi.IngestDesc


def desc(fmt, w, h, crop=(0, 0, 0, 0), colors=BW, double=OFF):
    return Desc(fmt, colors, double, 0, crop[0], crop[1], crop[2], crop[3], w, h)


bind = abi.bind


def emu(emu_lib):
    """the emulator build through device_calls' handle, with the ingest entries bound"""
    return bind(dc.emu_lib_of(emu_lib))


def product():
    return bind(dc.product_lib())


def geometry(lib, d):
    """(rc, out_width, out_height, doubled, src_row_bytes)"""
    ow, oh, dbl, rb = C.c_int(-1), C.c_int(-1), C.c_int(-1), C.c_size_t(0)
    rc = lib.sdv_ingest_geometry(C.byref(d), C.byref(ow), C.byref(oh), C.byref(dbl), C.byref(rb))
    return rc, ow.value, oh.value, dbl.value, rb.value


# ---- the header's text ------------------------------------------------------------------------------------------------------------------------
def row_bytes(fmt, w):
    if fmt == GRAY8:
        return w
    if fmt in (UYVY422, YUYV422):
        return 4 * ((w + 1) // 2)        # two pixels to a 4-byte macropixel
    if fmt == V210:
        return 16 * ((w + 5) // 6)
    if fmt == GRAY10LE:
        return 2 * w
    return (3 if fmt in (RGB24, BGR24) else 4) * w


def needs_double(width):
    return 10 < width < 959      # MIN_DBL_WIDTH / MAX_DBL_WIDTH


def samples(rows, fmt, w, colors=BW):
    """rows: (n, h, row bytes) uint8 -> the 8-bit sample of every source pixel, (n, h, w)"""
    n, h, _ = rows.shape
    if fmt == GRAY8:
        return rows[:, :, :w]
    if fmt == UYVY422:
        return rows[:, :, 1::2][:, :, :w]
    if fmt == YUYV422:
        return rows[:, :, 0::2][:, :, :w]
    if fmt == V210:
        words = np.ascontiguousarray(rows).view("<u4").reshape(n, h, -1, 4)                      # groups of four words
        comps = np.stack([words & 0x3FF, (words >> 10) & 0x3FF, (words >> 20) & 0x3FF], axis=-1).reshape(n, h, -1, 12)
        return (comps[:, :, :, 1::2].reshape(n, h, -1)[:, :, :w] >> 2).astype(np.uint8)
    if fmt == GRAY10LE:
        return ((np.ascontiguousarray(rows).view("<u2")[:, :, :w] & 0x3FF) >> 2).astype(np.uint8)
    bpp = 3 if fmt in (RGB24, BGR24) else 4
    px = rows[:, :, :bpp * w].reshape(n, h, w, bpp).astype(np.uint32)
    r, g, b = (px[..., 0], px[..., 1], px[..., 2]) if fmt in (RGB24, RGB0) else (px[..., 2], px[..., 1], px[..., 0])
    if colors == BW:
        return ((77 * r + 150 * g + 29 * b + 128) >> 8).astype(np.uint8)
    return (r, g, b)[colors - 1].astype(np.uint8)


def gather_rows(src, rb, h, n, srs, sfs):
    """the rows of the frames in the byte array `src` (from the pointer the call gets): (n, h, rb)"""
    idx = np.arange(n)[:, None, None] * sfs + np.arange(h)[None, :, None] * srs + np.arange(rb)[None, None, :]
    return src[idx]


def ingest_ref(src, fmt, w, h, n, srs, sfs, crop=(0, 0, 0, 0), colors=BW, double=OFF):
    """-> (luma (n, out_h, out_w) uint8, doubled)"""
    left, right, top, bottom = crop
    y = samples(gather_rows(src, row_bytes(fmt, w), h, n, srs, sfs), fmt, w, colors)
    if h > MAX_LINES:
        bottom = h - MAX_LINES
    y = y[:, top:h - bottom, left:w - right]
    doubled = needs_double(y.shape[2]) if double == AUTO else double == ON
    if doubled:
        y = np.repeat(y, 2, axis=2)
    return np.ascontiguousarray(y), int(doubled)


# ---- a luma plane hidden in a packed format ---------------------------------------------------------------------------------------------------
def pack(fmt, luma, rng):
    """(n, h, w) uint8 -> (n, h, row bytes) uint8 whose samples are `luma`; everything the sample does not depend on is random"""
    n, h, w = luma.shape
    rb = row_bytes(fmt, w)
    rows = rng.integers(0, 256, size=(n, h, rb), dtype=np.uint8)
    if fmt == GRAY8:
        rows[:, :, :w] = luma
    elif fmt in (UYVY422, YUYV422):
        at = 1 if fmt == UYVY422 else 0
        rows[:, :, at:2 * w:2] = luma
    elif fmt == V210:
        groups = rb // 16
        comps = rng.integers(0, 1024, size=(n, h, groups, 12), dtype=np.uint32)
        y = comps[:, :, :, 1::2].reshape(n, h, -1).copy()
        y[:, :, :w] = (luma.astype(np.uint32) << 2) | rng.integers(0, 4, size=luma.shape, dtype=np.uint32)
        comps[:, :, :, 1::2] = y.reshape(n, h, groups, 6)
        c = comps.reshape(n, h, groups, 4, 3)
        words = c[..., 0] | c[..., 1] << 10 | c[..., 2] << 20 | rng.integers(0, 4, size=c.shape[:-1], dtype=np.uint32) << 30
        rows = words.astype("<u4").reshape(n, h, -1).view(np.uint8).reshape(n, h, rb)
    elif fmt == GRAY10LE:
        v = (luma.astype(np.uint16) << 2) | rng.integers(0, 4, size=luma.shape, dtype=np.uint16) | (rng.integers(0, 64, size=luma.shape, dtype=np.uint16) << 10)
        rows = v.astype("<u2").view(np.uint8).reshape(n, h, rb)
    else:
        bpp = 3 if fmt in (RGB24, BGR24) else 4
        rows.reshape(n, h, w, bpp)[..., :3] = luma[..., None]
    return np.ascontiguousarray(rows)


# ---- one call ---------------------------------------------------------------------------------------------------------------------------------
def run_case(via, lib, eng, rng, fmt, w, h, n=1, crop=(0, 0, 0, 0), colors=BW, double=OFF, src_off=0, src_pad=0, dst_off=0, dst_pad=0, frame_pad=0, rows=None):
    """One sdv_ingest_frames call on random bytes (or on `rows`, (n, h, row bytes)) in buffers with the given offsets and paddings: asserts the
    geometry, the return code and EVERY byte of the destination buffer -> (luma, doubled)."""
    rb = row_bytes(fmt, w)
    srs = rb + src_pad
    sfs = h * srs + frame_pad
    raw = rng.integers(0, 256, size=src_off + (n - 1) * sfs + (h - 1) * srs + rb, dtype=np.uint8)
    if rows is not None:
        idx = src_off + np.arange(n)[:, None, None] * sfs + np.arange(h)[None, :, None] * srs + np.arange(rb)[None, None, :]
        raw[idx] = rows
    d = desc(fmt, w, h, crop, colors, double)
    want, doubled = ingest_ref(raw[src_off:], fmt, w, h, n, srs, sfs, crop, colors, double)
    _, oh, ow = want.shape
    assert geometry(lib, d) == (OK, ow, oh, doubled, rb)
    drs = ow + dst_pad
    dfs = oh * drs + frame_pad
    span = (n - 1) * dfs + (oh - 1) * drs + ow
    expect = np.full(dst_off + span + TAIL, FILL, dtype=np.uint8)
    sbuf, dbuf = via.array(raw), via.array(expect.copy())
    rc = lib.sdv_ingest_frames(eng, C.byref(d), via.ptr(sbuf, src_off), srs, sfs, n, via.ptr(dbuf, dst_off), drs, dfs, via.stream())
    assert rc == OK, lib.sdv_last_error(eng)
    got = via.get(dbuf)                 # (DEVICE: also the guard behind the buffer)
    expect[dst_off + np.arange(n)[:, None, None] * dfs + np.arange(oh)[None, :, None] * drs + np.arange(ow)[None, None, :]] = want
    if not np.array_equal(got, expect):
        bad = np.flatnonzero(got != expect)
        raise AssertionError("%d bytes differ, the first at %d of the destination buffer (rows start at %d, stride %d, %d bytes each; %d behind them)"
                             % (len(bad), bad[0], dst_off, drs, ow, TAIL))
    assert np.array_equal(via.get(sbuf), raw)           # the source is read only
    return want, doubled
