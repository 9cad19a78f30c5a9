"""out_fmt of sdv_encode_frames / sdv_encode_markerless_frames: the encoders write UYVY / YUY2, v210, a 10-bit plane or RGB / BGR rows straight from the
raster kernel (csrc/encode_packed_device.h).

The expected luma planes are encode_api.tape_words / tape_frames and encode_markerless_api.tape_bits / frames_of_bits, the expected bytes
encode_packed_api.pack_ref of them - numpy written from the header's text, never the code under test; the comparison is bytewise and covers the
whole destination buffer: the rows, the padding of every row, the bytes in front of and behind the stated span (on the GPU also device_calls'
guard).  Every body is written once against a memory of device_calls.py and called by a test_emu_* / test_gpu_* pair (tests/test_twins.py)."""
import ctypes as C
import functools

import numpy as np
import pytest

import device_calls as dc
import encode_api as en
import encode_markerless_api as ml
import encode_packed_api as ep
import pcm16_api as p16
import stitch_api as sa
from sdvpcmdecoder_amd import abi

STC007, PCM16X0 = abi.PCM_STC007, abi.PCM_PCM16X0
FMT_NAMES = sorted(ep.PACKED, key=ep.PACKED.get)
TC = (1, 2, 3, 4, 5)


def _engine(lib):
    eng = C.c_void_p(lib.sdv_engine_create(0))
    assert eng, lib.sdv_last_error(None)
    return eng


def _audio(rng, n_pairs, res=en.BIT16):
    pcm = rng.integers(-32768, 32768, size=(n_pairs, 2), dtype=np.int16)
    return pcm & ~3 if res == en.BIT14 else pcm         # (14 bit: what the truncation keeps)


# ---- the five encoders of the suite, each with two frames of seeded audio and their lines, made once ----------------------------------------------
ENCODERS = ("stc_ntsc_14bit_ctrl", "stc_pal_16bit", "pcm1", "pcm16x0_si", "pcm16x0_ei")
_STC = {"stc_ntsc_14bit_ctrl": (en.NTSC, en.BIT14, 1), "stc_pal_16bit": (en.PAL, en.BIT16, 0)}
_ML = {"pcm1": (ml.PCM1, 1, 0), "pcm16x0_si": (ml.SI, 0, ml.RATE_44100), "pcm16x0_ei": (ml.EI, 0, ml.EMPHASIS)}


@functools.lru_cache(maxsize=None)
def _two_frames(enc):
    """(pcm of two frames, the lines of the two frames, lines per field) of an encoder; shared by the cases, never written to"""
    rng = np.random.default_rng(100 + ENCODERS.index(enc))
    if enc in _STC:
        std, res, ctrl = _STC[enc]
        pcm = _audio(rng, 2 * en.pairs_per_frame(std), res)
        return pcm, en.tape_words(pcm, 2, std, res, ctrl, 0, TC), en.LPF[std] + ctrl
    fmt, header, flags = _ML[enc]
    pcm = _audio(rng, 2 * ml.PAIRS_PER_FRAME)
    return pcm, ml.tape_bits(pcm, 2, fmt, header, flags), ml.LINES + header


def _desc_and_planes(enc, order, black, white, width, height, start, stop, top):
    """(descriptor with out_fmt 0, the two luma planes it asks for (2, height, width))"""
    _, lines, _ = _two_frames(enc)
    if enc in _STC:
        std, res, ctrl = _STC[enc]
        d = en.desc(std, res, ctrl, 0, order, black, white, TC, width, height, start, stop, top)
        return d, en.tape_frames(lines, d)
    fmt, header, flags = _ML[enc]
    d = ml.desc(fmt, order, black, white, header, flags, width, height, start, stop, top)
    return d, ml.frames_of_bits(lines, d)


# ---- 1. formats and edges -----------------------------------------------------------------------------------------------------------------------
WIDTHS = (1, 2, 5, 6, 7, 11, 12, 13, 15, 16, 17, 31, 33, 137)      # every residue modulo 6, both parities, around a unit of 16 pixels, several units
CASES_PER_FORMAT = 28                                               # 8 formats x 28 = 224 cases: every (width, format) pair twice


def _window(kind, w):
    """inside the picture, touching its edges, reaching past both, narrower than 69 pixels (pixel by pixel: `narrow`), and so far past both that
    even a narrow picture shows cells less than 32 apart (the windowed lookup)"""
    if kind == 0:
        return w // 4, max(w // 4 + 1, w - w // 4)
    if kind == 1:
        return 0, w
    if kind == 2:
        return -(1 + w // 3), w + 2 + w // 5
    if kind == 3:
        return w // 5, w // 5 + max(1, min(40, w // 2))
    return -300 - w, w + 400


def _formats_and_edges(lib, via, fmt_name):
    """A seeded sample of the cross product for one format: the widths cycle (with the format of the parametrisation every pair occurs twice) and so
    do the five encoders; drawn: the window (five kinds), heights 1 / 5 / 6, a top_line of 0, -1 (the first two rows without a line), the last but
    one line (rows behind it without one) or beyond the field (an all-black frame), field order, levels, destination offset 0 / 1 / 3 / 6, row
    padding 0 / 6, frame padding 0 / 10, pcm offset 0 / 2.  Two frames a case; every case is a tape of its own."""
    fmt = ep.PACKED[fmt_name]
    rng = np.random.default_rng(3000 + fmt)
    eng = _engine(lib)
    try:
        for i in range(CASES_PER_FORMAT):
            width = WIDTHS[i % len(WIDTHS)]
            enc = ENCODERS[(i + fmt) % len(ENCODERS)]
            pcm, _, lpft = _two_frames(enc)
            height = int(rng.choice((1, 5, 6)))
            start, stop = _window(int(rng.integers(0, 5)), width)
            top = int(rng.choice((0, -1, lpft - 2, lpft + 5)))
            black = int(rng.integers(0, 255))
            d, planes = _desc_and_planes(enc, int(rng.integers(0, 2)), black, int(rng.integers(black + 1, 256)), width, height, start, stop, top)
            if top > lpft:
                assert (planes == black).all()
            ep.with_fmt(d, fmt)
            pairs, lines, rb = ep.geometry(lib, d)[1:]
            assert (ep.geometry(lib, d)[0], 2 * pairs, lines, rb) == (ep.OK, len(pcm), lpft, ep.row_bytes(fmt, width))
            assert lib.sdv_reset_encoder(eng) == en.OK
            ep.run_call(via, lib, eng, d, pcm, len(pcm), 2, planes, dst_off=int(rng.choice((0, 1, 3, 6))), dst_pad=int(rng.choice((0, 6))),
                        frame_pad=int(rng.choice((0, 10))), pcm_off=int(rng.choice((0, 2))))
    finally:
        lib.sdv_engine_destroy(eng)


@pytest.mark.parametrize("fmt_name", FMT_NAMES)
def test_emu_formats_and_edges(fmt_name, emu_lib):
    _formats_and_edges(en.emu(emu_lib), dc.HOST, fmt_name)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt_name", FMT_NAMES)
def test_gpu_formats_and_edges(fmt_name):
    _formats_and_edges(en.product(), dc.DEVICE, fmt_name)


# ---- 2. back through ingest ---------------------------------------------------------------------------------------------------------------------
def _ingest(via, lib, eng, packed, fmt, width, height, n):
    """sdv_ingest_frames of contiguous packed rows (n, height, row bytes) with the same format, SDV_COLOR_BW, no crop, no doubling -> (n, height, width)"""
    rb = packed.shape[2]
    d = abi.IngestDesc(fmt, abi.COLOR_BW, abi.INGEST_DOUBLE_OFF, 0, 0, 0, 0, 0, width, height)
    sbuf, dbuf = via.array(np.ascontiguousarray(packed).reshape(-1)), via.array(np.full(n * height * width, en.FILL, dtype=np.uint8))
    rc = lib.sdv_ingest_frames(eng, C.byref(d), via.ptr(sbuf), rb, height * rb, n, via.ptr(dbuf), width, height * width, via.stream())
    assert rc == ep.OK, lib.sdv_last_error(eng)
    return via.get(dbuf).reshape(n, height, width)


def _back_through_ingest(lib, via, fmt_name):
    """Widths 7, 13 and 137, two frames of height 6: what sdv_ingest_frames makes of the packed frames equals the bytes a fresh engine's GRAY8 call
    makes from the same PCM."""
    fmt = ep.PACKED[fmt_name]
    pcm, lines, _ = _two_frames("stc_ntsc_14bit_ctrl")
    for width in (7, 13, 137):
        d = en.desc(en.NTSC, en.BIT14, 1, 0, en.TFF, 16, 235, TC, width, 6, -2, width + 3, 100)
        planes = en.tape_frames(lines, d)
        plain, packing = _engine(lib), _engine(lib)
        try:
            gray = en.frames_of(en.run_call(via, lib, plain, d, pcm, len(pcm), 2, planes), d, 2)
            rb = ep.row_bytes(fmt, width)
            packed = ep.rows_of(ep.run_call(via, lib, packing, ep.with_fmt(d, fmt), pcm, len(pcm), 2, planes), rb, 6, 2)
            assert np.array_equal(_ingest(via, lib, packing, packed, fmt, width, 6, 2), gray)
        finally:
            lib.sdv_engine_destroy(plain)
            lib.sdv_engine_destroy(packing)


@pytest.mark.parametrize("fmt_name", FMT_NAMES)
def test_emu_back_through_ingest(fmt_name, emu_lib):
    _back_through_ingest(en.emu(emu_lib), dc.HOST, fmt_name)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt_name", FMT_NAMES)
def test_gpu_back_through_ingest(fmt_name):
    _back_through_ingest(en.product(), dc.DEVICE, fmt_name)


# ---- 3. streaming -------------------------------------------------------------------------------------------------------------------------------
def _streaming(lib, via):
    """One tape of 5 frames in calls of 1, 2, 0 and 2 frames whose out_fmt differs from call to call equals the one-call tape packed frame by frame:
    the tape's state does not depend on out_fmt.  Calls refused for their out_fmt in between write nothing and leave the tape where it was."""
    rng = np.random.default_rng(9)
    eng = _engine(lib)
    std, res, tc = en.NTSC, en.BIT14, (3, 15, 59, 59, 47)
    ppf = en.pairs_per_frame(std)
    pcm = _audio(rng, 5 * ppf - 700, res)

    def desc(fmt, reserved=0, at=1):
        return ep.with_fmt(en.desc(std, res, 1, en.EMPHASIS, en.TFF, 30, 200, tc, 97, 30, 3, 95, 0), fmt, reserved, at)
    planes = en.tape_frames(en.tape_words(pcm, 5, std, res, 1, en.EMPHASIS, tc), desc(0))
    try:
        done = 0
        for n, fmt in ((1, ep.UYVY422), (2, ep.V210), (0, ep.RGB24), (2, ep.BGR0)):
            left = pcm[done * ppf:]
            ep.run_call(via, lib, eng, desc(fmt), left, len(left), n, planes[done:done + n], dst_off=3, dst_pad=6)
            done += n
            for bad in (desc(9), desc(ep.GRAY10LE, 1, 2)):
                ep.run_call(via, lib, eng, bad, left, len(left), 1, None, expect_rc=ep.BAD_ARG, drs=4 * 97, dfs=4 * 97 * 30)
                assert b"out_fmt" in lib.sdv_last_error(eng)
        assert done == 5
    finally:
        lib.sdv_engine_destroy(eng)


def test_emu_streaming(emu_lib):
    _streaming(en.emu(emu_lib), dc.HOST)


@pytest.mark.gpu
def test_gpu_streaming():
    _streaming(en.product(), dc.DEVICE)


# ---- 4. it decodes ------------------------------------------------------------------------------------------------------------------------------
DECODES = {"stc007_v210": ("stc_ntsc_14bit_ctrl", ep.V210), "stc007_uyvy422": ("stc_ntsc_14bit_ctrl", ep.UYVY422), "stc007_rgb24": ("stc_ntsc_14bit_ctrl", ep.RGB24),
           "pcm16x0_si_bgr0": ("pcm16x0_si", ep.BGR0)}


def _it_decodes(lib, via, case):
    """The ntsc_14bit_ctrl shape of tests/test_encode.py (3 frames of 720 x 492, the last from no pairs) as v210, as uyvy422 and as rgb24 (a build
    whose lanes share units, at a width where its lookup goes by the window), and the pcm16_si shape of tests/test_encode_markerless.py (3 frames of
    720 x 490) as bgr0: the packed frames go through sdv_ingest_frames and then
    sdv_decode_frames(NEW_FILE | END_FILE) as they lie in the memory of the calls; every source pair comes back in order with
    SDV_SF_BLOCK_OK | SDV_SF_WORD_VALID on both channels."""
    enc, fmt = DECODES[case]
    rng = np.random.default_rng(77)
    n = 3
    if enc in _STC:
        std, res, ctrl = _STC[enc]
        d = ep.with_fmt(en.desc(std, res, ctrl, 0, en.TFF, 30, 200, (2, 1, 2, 59, 58), 720, 492, 12, 708, 0), fmt)
        pcm = _audio(rng, 2 * en.pairs_per_frame(std), res)
        pcm_type, frasm = STC007, sa.FRASM_DTYPE
    else:
        d = ep.with_fmt(ml.desc(ml.SI, ml.TFF, 30, 200, 0, ml.RATE_44100, 720, 490, 4, 716, 0), fmt)
        pcm = _audio(rng, n * ml.PAIRS_PER_FRAME)
        pcm_type, frasm = PCM16X0, p16.FRASM16_DTYPE
    h, rb = d.height, ep.row_bytes(fmt, 720)
    eng = _engine(lib)
    try:
        packed = via.array(np.full(n * h * rb, en.FILL, dtype=np.uint8))
        luma = via.array(np.full(n * h * 720, en.FILL, dtype=np.uint8))
        sbuf = via.array(pcm)
        assert ep.frames_call(lib, d)(eng, C.byref(d), via.ptr(sbuf), len(pcm), n, via.ptr(packed), rb, rb * h, via.stream()) == ep.OK, lib.sdv_last_error(eng)
        ing = abi.IngestDesc(fmt, abi.COLOR_BW, abi.INGEST_DOUBLE_OFF, 0, 0, 0, 0, 0, 720, h)
        assert lib.sdv_ingest_frames(eng, C.byref(ing), via.ptr(packed), rb, rb * h, n, via.ptr(luma), 720, 720 * h, via.stream()) == ep.OK, lib.sdv_last_error(eng)
        lib.sdv_set_pcm_type(eng, pcm_type, 0)
        if pcm_type == PCM16X0:
            st = p16.default_settings(format=p16.FORMAT_SI, field_order=1)
            assert lib.sdv_set_pcm16x0_stitch_settings(eng, C.byref(st)) == 0
        cap = (n + 2) * 2100 + 8192
        pairs, frames = via.zeros(cap, sa.PAIR_DTYPE), via.zeros(n + 16, frasm)
        n_pairs, n_frames = C.c_size_t(0), C.c_size_t(0)
        rc = lib.sdv_decode_frames(eng, pcm_type, via.ptr(luma), 720, 720 * h, 720, h, n, 1, 1 | 4, via.ptr(pairs), cap, C.byref(n_pairs),
                                   via.ptr(frames), len(frames), C.byref(n_frames), None, 0, 0, 0, None, 0, None, None, via.stream())
        assert rc == 0, lib.sdv_last_error(eng)
        got_p = via.get(pairs, n_pairs.value)
    finally:
        lib.sdv_engine_destroy(eng)
    audio = got_p[got_p["service_type"] == 0]
    if enc in _STC:             # behind the decoder's lead-in
        first = next((k for k in range(len(audio) - len(pcm) + 1) if np.array_equal(audio["audio_word"][k:k + 8], pcm[:8])), None)
        assert first is not None and first < 2 * 112 * 3
    else:
        first = 0
        assert len(audio) == len(pcm)
    assert np.array_equal(audio["audio_word"][first:first + len(pcm)], pcm)
    assert ((audio["sample_flags"][first:first + len(pcm)] & 3) == 3).all()           # SDV_SF_BLOCK_OK | SDV_SF_WORD_VALID


@pytest.mark.parametrize("case", sorted(DECODES))
def test_emu_it_decodes(case, emu_lib):
    _it_decodes(en.emu(emu_lib), dc.HOST, case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(DECODES))
def test_gpu_it_decodes(case):
    _it_decodes(en.product(), dc.DEVICE, case)


# ---- 5. more than one trip ----------------------------------------------------------------------------------------------------------------------
def _more_than_one_trip(lib, via):
    """1100 frames of 137 x 54 as gray10le at a destination 3 bytes off: 1100 x 54 x 9 units of 16 pixels, more than the 2048 x 256 threads of the
    product's launch, so its threads take a second trip with the stride split into frames, rows and units for that launch size (the emulator build
    walks every case with a few threads); every row is 3 bytes off a 16-byte boundary."""
    rng = np.random.default_rng(13)
    n, d = 1100, ep.with_fmt(en.desc(en.NTSC, en.BIT14, 0, 0, en.TFF, 16, 235, (0, 0, 0, 0, 0), 137, 54, 0, 137, 100), ep.GRAY10LE)
    assert n * 54 * ((137 + 15) // 16) > 2048 * 256
    pcm = _audio(rng, n * en.pairs_per_frame(en.NTSC), en.BIT14)
    eng = _engine(lib)
    try:
        ep.run_call(via, lib, eng, d, pcm, len(pcm), n, en.tape_frames(en.tape_words(pcm, n), d), dst_off=3)
    finally:
        lib.sdv_engine_destroy(eng)


def test_emu_more_than_one_trip(emu_lib):
    _more_than_one_trip(en.emu(emu_lib), dc.HOST)


@pytest.mark.gpu
def test_gpu_more_than_one_trip():
    _more_than_one_trip(en.product(), dc.DEVICE)


# ---- 6. refusals and geometry -------------------------------------------------------------------------------------------------------------------
def _refusals(lib, via):
    """Host checks ahead of any launch: the code, a reason in sdv_last_error, the destination untouched, the same code from the geometry call where
    the descriptor alone is at fault, and the tape where it was - the good call behind every refusal writes the next frame of one tape, as UYVY."""
    rng = np.random.default_rng(17)
    eng = _engine(lib)
    w, h, n = 40, 6, 2
    ppf = en.pairs_per_frame(en.NTSC)
    pcm = _audio(rng, 20 * ppf, en.BIT14)

    def stc(fmt, reserved=0, at=1):
        return ep.with_fmt(en.desc(en.NTSC, en.BIT14, 1, 0, en.TFF, 30, 200, TC, w, h, 2, 38, 0), fmt, reserved, at)

    def mless(fmt, reserved=0):
        return ep.with_fmt(ml.desc(ml.SI, ml.TFF, 30, 200, 0, 0, w, h, 2, 38, 0), fmt, reserved, 1)
    good = stc(ep.UYVY422)
    rb = ep.row_bytes(ep.UYVY422, w)
    assert rb == 80
    tape = ep.pack_ref(en.tape_frames(en.tape_words(pcm, 20, en.NTSC, en.BIT14, 1, 0, TC), good), ep.UYVY422, 30)
    src = via.array(pcm)
    dst = via.array(np.full(8192, en.FILL, dtype=np.uint8))
    sp, dp = via.ptr(src), via.ptr(dst)
    done = [0]

    def refused(d, geo, s=sp, t=dp, drs=4 * w, dfs=4 * w * h):
        assert ep.frames_call(lib, d)(eng, C.byref(d), s, n * ppf, n, t, drs, dfs, via.stream()) == ep.BAD_ARG
        why = lib.sdv_last_error(eng)
        assert why and (not geo or b"out_fmt" in why), why
        assert (via.get(dst) == en.FILL).all()
        assert ep.geometry(lib, d)[0] == (ep.BAD_ARG if geo else ep.OK)
        if geo:
            assert b"out_fmt" in lib.sdv_last_error(None)
        out = via.array(np.full(h * rb + en.TAIL, en.FILL, dtype=np.uint8))            # ... and the engine takes the next call, on the same tape
        assert lib.sdv_encode_frames(eng, C.byref(good), via.ptr(src, 2 * ppf * done[0]), ppf, 1, via.ptr(out), rb, h * rb, via.stream()) == ep.OK
        got = via.get(out)
        assert np.array_equal(got[:h * rb], tape[done[0]].reshape(-1)) and (got[h * rb:] == en.FILL).all()
        done[0] += 1
    try:
        # what out_fmt cannot say, for either encoder
        for make in (stc, mless):
            refused(make(9), True)
            refused(make(255), True)
            refused(make(ep.UYVY422, 1), True)
            refused(make(ep.GRAY8, 7), True)
        refused(stc(ep.V210, 1, 2), True)
        # strides: one short of the 80 bytes of a row; `width`, which GRAY8 takes; a frame stride one short
        for make in (stc, mless):
            refused(make(ep.UYVY422), False, drs=rb - 1, dfs=h * rb)
            refused(make(ep.UYVY422), False, drs=w, dfs=h * rb)
            refused(make(ep.UYVY422), False, drs=rb, dfs=(h - 1) * rb + rb - 1)
            assert b"dst_" in lib.sdv_last_error(eng)
        d8 = stc(ep.GRAY8)
        assert lib.sdv_encode_frames(eng, C.byref(d8), sp, 0, 1, dp, w, h * w, via.stream()) == ep.OK       # (a stride of `width` is GRAY8's; this is frame `done` of the tape)
        got = via.get(dst)
        assert (got[h * w:] == en.FILL).all() and not (got[:h * w] == en.FILL).all()
        dst = via.array(np.full(8192, en.FILL, dtype=np.uint8))
        dp = via.ptr(dst)
        # an overlap that only the packed span has: the last byte of the 4-byte rows on the first byte of the pairs, where the plane would end 480 bytes short of them
        span = (n - 1) * 4 * w * h + (h - 1) * 4 * w + 4 * w
        assert span == 4 * n * h * w
        assert lib.sdv_encode_frames(eng, C.byref(stc(ep.RGB0)), dp + 2048, n * ppf, n, dp + 2048 - span + 1, 4 * w, 4 * w * h, via.stream()) == ep.BAD_ARG
        assert b"overlap" in lib.sdv_last_error(eng) and (via.get(dst) == en.FILL).all()
        assert lib.sdv_encode_markerless_frames(eng, C.byref(mless(ep.BGR0)), dp + 2048, n * ppf, n, dp + 2048 - span + 1, 4 * w, 4 * w * h, via.stream()) == ep.BAD_ARG
        assert b"overlap" in lib.sdv_last_error(eng) and (via.get(dst) == en.FILL).all()
        # the bytes of a row
        for width, want in ((720, {ep.UYVY422: 1440, ep.YUYV422: 1440, ep.V210: 1920, ep.GRAY10LE: 1440, ep.RGB24: 2160, ep.BGR24: 2160, ep.RGB0: 2880, ep.BGR0: 2880, ep.GRAY8: 720}),
                            (721, {ep.UYVY422: 1444, ep.V210: 1936})):
            for fmt, row in want.items():
                assert ep.geometry(lib, ep.with_fmt(en.desc(width=width), fmt))[3] == row == ep.row_bytes(fmt, width)
                assert ep.geometry(lib, ep.with_fmt(ml.desc(width=width), fmt))[3] == row
    finally:
        lib.sdv_engine_destroy(eng)


def test_emu_refusals(emu_lib):
    _refusals(en.emu(emu_lib), dc.HOST)


@pytest.mark.gpu
def test_gpu_refusals():
    _refusals(en.product(), dc.DEVICE)


# ---- 7. the library, the wrapper, the host program ------------------------------------------------------------------------------------------------
def test_abi_version_and_geometry_of_the_product_library():
    from sdvpcmdecoder_amd import build as b
    lib = en.bind(C.CDLL(b.build_hip()))
    assert lib.sdv_abi_version() >= 12
    assert en.geometry(lib, ep.with_fmt(en.desc(en.NTSC, ctrl=1), ep.V210)) == (0, 1470, 246, 1920)
    assert ml.geometry(lib, ep.with_fmt(ml.desc(ml.PCM1, header=1), ep.RGB24)) == (0, 1470, 246, 2160)
    assert en.geometry(lib, ep.with_fmt(en.desc(), 9))[0] == ep.BAD_ARG and b"out_fmt" in lib.sdv_last_error(None)


@pytest.mark.gpu
def test_gpu_work_runs_on_the_stream_it_is_given():
    """The PCM buffer holds tape B; a non-blocking side stream is kept busy, copies tape A in and gets the call; the output is cloned on that
    stream.  Work of the call on any other stream reads tape B, or is read half written."""
    import torch
    lib = en.product()
    rng = np.random.default_rng(41)
    n = 2
    d = ep.with_fmt(en.desc(ctrl=1, height=492), ep.UYVY422)
    rb = ep.row_bytes(ep.UYVY422, 720)
    pcm_a, pcm_b = _audio(rng, n * 1470, en.BIT14), _audio(rng, n * 1470, en.BIT14)
    want = ep.pack_ref(en.tape_frames(en.tape_words(pcm_a, n, ctrl=1), d), ep.UYVY422, d.black)
    eng = _engine(lib)
    try:
        side = torch.cuda.Stream()
        assert side.cuda_stream != 0
        buf = torch.from_numpy(pcm_b.copy()).cuda()
        pinned = torch.from_numpy(pcm_a.copy()).pin_memory()
        out = torch.full((want.size,), en.FILL, dtype=torch.uint8, device="cuda")
        ballast = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
        # what an engine allocates in its first call is part of that call: made ahead, on tape B, then a new tape
        assert lib.sdv_encode_frames(eng, C.byref(d), C.c_void_p(buf.data_ptr()), len(pcm_b), n, C.c_void_p(out.data_ptr()), rb, rb * 492, None) == ep.OK
        assert lib.sdv_reset_encoder(eng) == ep.OK
        torch.cuda.synchronize()
        out.fill_(en.FILL)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            for v in range(4):
                ballast.fill_(v)
            buf.copy_(pinned, non_blocking=True)
        rc = lib.sdv_encode_frames(eng, C.byref(d), C.c_void_p(buf.data_ptr()), len(pcm_a), n, C.c_void_p(out.data_ptr()), rb, rb * 492, C.c_void_p(side.cuda_stream))
        assert rc == ep.OK, lib.sdv_last_error(eng)
        with torch.cuda.stream(side):
            got = out.clone()
        side.synchronize()
        assert np.array_equal(got.cpu().numpy(), want.reshape(-1))
        torch.cuda.synchronize()
    finally:
        lib.sdv_engine_destroy(eng)


@pytest.mark.gpu
def test_gpu_engine_wrapper():
    """Engine.encode_frames / encode_markerless_frames with pix_fmt: an (n, height, row_bytes) uint8 tensor on torch's current stream, by name or by
    value; Engine.ingest takes it back to the plane of the plain call; a pix_fmt the library refuses is a RuntimeError."""
    import torch
    from sdvpcmdecoder_amd import Engine
    rng = np.random.default_rng(31)
    pcm = _audio(rng, 2 * 1470, en.BIT14)
    d = en.desc(ctrl=1, height=492)
    planes = en.tape_frames(en.tape_words(pcm, 3, ctrl=1), d)
    eng = Engine(0)
    t = torch.from_numpy(pcm).cuda()
    a = eng.encode_frames(t[:1470], 1, ctrl_block=True, height=492, pix_fmt="v210")
    b = eng.encode_frames(t[1470:], 2, ctrl_block=True, height=492, pix_fmt=abi.PIX_RGB0)
    assert a.shape == (1, 492, 1920) and b.shape == (2, 492, 2880) and a.dtype == b.dtype == torch.uint8
    assert np.array_equal(a.cpu().numpy(), ep.pack_ref(planes[:1], ep.V210, 30)) and np.array_equal(b.cpu().numpy(), ep.pack_ref(planes[1:], ep.RGB0, 30))
    eng.reset_encoder()
    plain = eng.encode_frames(t, 3, ctrl_block=True, height=492)
    assert plain.shape == (3, 492, 720) and np.array_equal(plain.cpu().numpy(), planes)
    back, doubled = eng.ingest(a, "v210", 720, 492, double="off")
    assert not doubled and np.array_equal(back[0].cpu().numpy(), planes[0])
    m = eng.encode_markerless_frames(t[:1470], 1, "pcm16x0_si", rate_44100=True, pix_fmt="uyvy422")
    dm = ml.desc(ml.SI, ctrl_flags=ml.RATE_44100)
    assert m.shape == (1, 490, 1440) and np.array_equal(m.cpu().numpy(), ep.pack_ref(ml.tape_frames(pcm[:1470], 1, dm), ep.UYVY422, 30))
    assert eng.encode_markerless_geometry(eng.encode_markerless_desc("pcm1", header_lines=1, height=492, pix_fmt="gray10le")) == (1470, 246, 1440)
    with pytest.raises(RuntimeError, match="out_fmt"):
        eng.encode_frames(t, 1, ctrl_block=True, height=492, pix_fmt=9)
    with pytest.raises(RuntimeError, match="out_fmt"):
        eng.encode_markerless_frames(t, 1, "pcm1", pix_fmt=200)
    eng.reset_encoder()
    assert np.array_equal(eng.encode_frames(t, 3, ctrl_block=True, height=492, pix_fmt="gray8").cpu().numpy(), planes)


@pytest.mark.gpu
def test_gpu_cpp_host_program_encodes_v210_and_decodes(tmp_path):
    """decode_tape encode in.wav tape.v210 v210, then decode_tape ingest, then decode_tape wav: the file holds pack_ref of the tape, rows of the
    row_bytes the program prints, and the WAV that comes back holds the samples of the WAV that went in, behind the decoder's lead-in."""
    import subprocess
    from sdvpcmdecoder_amd import build as b
    exe = b.build_example()
    rng = np.random.default_rng(29)
    pcm = _audio(rng, 2 * 1470 + 321, en.BIT14)
    hdr = b"RIFF" + (36 + pcm.nbytes).to_bytes(4, "little") + b"WAVEfmt " + (16).to_bytes(4, "little") + (1).to_bytes(2, "little") + (2).to_bytes(2, "little") + \
        (44056).to_bytes(4, "little") + (44056 * 4).to_bytes(4, "little") + (4).to_bytes(2, "little") + (16).to_bytes(2, "little") + b"data" + pcm.nbytes.to_bytes(4, "little")
    (tmp_path / "in.wav").write_bytes(hdr + pcm.tobytes())
    out = subprocess.run([exe, "encode", str(tmp_path / "in.wav"), str(tmp_path / "tape.v210"), "v210"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr + out.stdout
    n, width, height, rb = (int(x) for x in out.stdout.split()[:4])
    assert (n, width, height, rb) == (4, 720, 492, 1920) and (tmp_path / "tape.v210").stat().st_size == n * rb * height
    want = en.tape_frames(en.tape_words(pcm, n, ctrl=1), en.desc(ctrl=1, height=492))
    assert (tmp_path / "tape.v210").read_bytes() == ep.pack_ref(want, ep.V210, 30).tobytes()
    out = subprocess.run([exe, "ingest", str(tmp_path / "tape.v210"), "v210", str(width), str(height), str(rb), str(n), "0,0,0,0", "bw", "off", str(tmp_path / "tape.luma")],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.split() == ["720", "492", "0"], out.stderr + out.stdout
    assert (tmp_path / "tape.luma").read_bytes() == want.tobytes()
    out = subprocess.run([exe, "wav", str(tmp_path / "tape.luma"), str(width), str(height), str(n), str(tmp_path / "back.wav")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr + out.stdout
    back = np.frombuffer((tmp_path / "back.wav").read_bytes()[44:], dtype=np.int16).reshape(-1, 2)
    first = next(k for k in range(len(back)) if np.array_equal(back[k:k + 8], pcm[:8]))
    assert np.array_equal(back[first:first + len(pcm)], pcm)
