"""sdv_ingest_frames / sdv_ingest_geometry: packed capture formats -> the luma plane of the frame entries, with crop, channel
pick and the integer 2x width doubling, on the device.

The expected bytes are ingest_api.ingest_ref, numpy written from the header's text; the comparison is bytewise and covers the whole destination
buffer: the rows, the padding of every row, the bytes in front of and behind the stated span (on the GPU also device_calls' guard).  Every body is
written once against a memory of device_calls.py and called by a test_emu_* / test_gpu_* pair (tests/test_twins.py)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import device_calls as dc
import ingest_api as ia
from oracle_run import oracle_binarize
from sdvpcmdecoder_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMAT_IDS = sorted(ia.FORMATS, key=ia.FORMATS.get)


def _engine(lib):
    eng = C.c_void_p(lib.sdv_engine_create(0))
    assert eng, lib.sdv_last_error(None)
    return eng


# ---- 1. every format, every edge --------------------------------------------------------------------------------------------------------------
WIDTHS = (1, 15, 16, 17, 31, 33, 137)       # out_width without doubling; with SDV_INGEST_DOUBLE_ON the kept width (out_width is twice that)
N_COMBINATIONS = 400


def _formats_and_edges(lib, via, fmt_name):
    """A seeded sample of the cross product: kept width x crop_left 0..7 (every residue mod 6 for v210, both parities for 4:2:2, a shifted
    16-byte phase) x doubling x crop_right {0, 5} x crop_top {0, 3} x crop_bottom {0, 2} x heights {1, 5} x 2 frames x source offset {0, 1, 2, 6}
    x source stride + {0, 6} x destination offset {0, 3} x destination stride + {0, 6}.  crop_left and the width cycle, so every pair of them
    occurs seven times; the rest is drawn.  With doubling a kept width of 8 (one whole 16-byte chunk) joins the list."""
    fmt = ia.FORMATS[fmt_name]
    rng = np.random.default_rng(1000 + fmt)
    eng = _engine(lib)
    try:
        for i in range(N_COMBINATIONS):
            double = (i // 56) % 2
            widths = WIDTHS + ((8,) if double else ())
            kept = widths[(i // 8) % len(widths)]
            left, right, top, bottom = i % 8, int(rng.choice((0, 5))), int(rng.choice((0, 3))), int(rng.choice((0, 2)))
            out_h = int(rng.choice((1, 5)))
            want, doubled = ia.run_case(via, lib, eng, rng, fmt, left + kept + right, top + out_h + bottom, n=2, crop=(left, right, top, bottom),
                                        double=double, src_off=int(rng.choice((0, 1, 2, 6))), src_pad=int(rng.choice((0, 6))),
                                        dst_off=int(rng.choice((0, 3))), dst_pad=int(rng.choice((0, 6))), frame_pad=int(rng.choice((0, 10))))
            assert want.shape == (2, out_h, kept * (2 if double else 1)) and doubled == double
    finally:
        lib.sdv_engine_destroy(eng)


@pytest.mark.parametrize("fmt_name", FORMAT_IDS)
def test_emu_formats_and_edges(fmt_name, emu_lib):
    _formats_and_edges(ia.emu(emu_lib), dc.HOST, fmt_name)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt_name", FORMAT_IDS)
def test_gpu_formats_and_edges(fmt_name):
    _formats_and_edges(ia.product(), dc.DEVICE, fmt_name)


# ---- 2. colour channels -----------------------------------------------------------------------------------------------------------------------
def _colour_channels(lib, via):
    """The four RGB formats x BW / R / G / B on random pixels with the extremes among them, through rows of several chunks, with and without
    doubling; a grey ramp comes out of BW unchanged."""
    rng = np.random.default_rng(7)
    eng = _engine(lib)
    extremes = np.array([(0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255)], dtype=np.uint8)
    w, h = 53, 3
    try:
        for fmt in ia.RGB_FORMATS:
            bpp = 3 if fmt in (ia.RGB24, ia.BGR24) else 4
            rgb = rng.integers(0, 256, size=(1, h, w, 3), dtype=np.uint8)
            rgb[0, 0, 20:25] = extremes                 # inside a whole chunk
            rgb[0, 1, :5] = extremes                    # at the head of a row
            rgb[0, 2, w - 5:] = extremes                # at its tail
            rows = rng.integers(0, 256, size=(1, h, w, bpp), dtype=np.uint8)
            rows[..., :3] = rgb if fmt in (ia.RGB24, ia.RGB0) else rgb[..., ::-1]
            for colors in (ia.BW, ia.R, ia.G, ia.B):
                for double in (ia.OFF, ia.ON):
                    want, _ = ia.run_case(via, lib, eng, rng, fmt, w, h, colors=colors, double=double, rows=rows.reshape(1, h, w * bpp), dst_off=1)
                    plane = want[:, :, ::2] if double else want
                    if colors == ia.BW:     # (the reference function itself at the extremes, by hand: (w * 255 + 128) >> 8 for the weights 77, 150, 29)
                        assert plane[0, 0, 20:25].tolist() == [0, 255, 77, 149, 29]
                    else:
                        assert np.array_equal(plane, rgb[..., colors - 1])
            ramp = np.arange(256, dtype=np.uint8).reshape(1, 1, 256)
            want, _ = ia.run_case(via, lib, eng, rng, fmt, 256, 1, colors=ia.BW, rows=ia.pack(fmt, ramp, rng))
            assert np.array_equal(want, ramp)
    finally:
        lib.sdv_engine_destroy(eng)


def test_emu_colour_channels(emu_lib):
    _colour_channels(ia.emu(emu_lib), dc.HOST)


@pytest.mark.gpu
def test_gpu_colour_channels():
    _colour_channels(ia.product(), dc.DEVICE)


# ---- 3. tall sources, many rows ---------------------------------------------------------------------------------------------------------------
def _tall_sources_and_many_rows(lib, via):
    """650 source lines: the bottom goes down to 640 whatever crop_bottom says (636 rows behind a crop_top of 4).  140 frames x 480 rows in one
    call: more rows than a grid dimension holds.  450 frames x 600 rows x 2 slots: more than one trip of the kernel's loop on the GPU."""
    rng = np.random.default_rng(11)
    eng = _engine(lib)
    try:
        for fmt in (ia.GRAY8, ia.V210, ia.RGB24):
            want, _ = ia.run_case(via, lib, eng, rng, fmt, 16, 650, crop=(0, 0, 4, 1))
            assert want.shape == (1, 636, 16)
        want, _ = ia.run_case(via, lib, eng, rng, ia.UYVY422, 24, 480, n=140)
        assert want.shape == (140, 480, 24) and 140 * 480 > 65535
        # more chunk slots than the product's launch has threads (2048 x 256): on the GPU the one case whose threads take a second trip, with the
        # stride split into frames, rows and slots for that launch size (the emulator build walks every case with a few threads)
        want, _ = ia.run_case(via, lib, eng, rng, ia.GRAY8, 16, 600, n=450, dst_off=3)
        assert want.shape == (450, 600, 16) and 450 * 600 * 2 > 2048 * 256
    finally:
        lib.sdv_engine_destroy(eng)


def test_emu_tall_sources_and_many_rows(emu_lib):
    _tall_sources_and_many_rows(ia.emu(emu_lib), dc.HOST)


@pytest.mark.gpu
def test_gpu_tall_sources_and_many_rows():
    _tall_sources_and_many_rows(ia.product(), dc.DEVICE)


# ---- 4. SDV_INGEST_DOUBLE_AUTO ----------------------------------------------------------------------------------------------------------------
def _auto_doubling(lib, via):
    """Cropped widths on both sides of MIN_DBL_WIDTH 10 and MAX_DBL_WIDTH 959: the geometry, the bytes and sdv_needs_double_width agree; the
    rule looks at the cropped width, not at the source's."""
    rng = np.random.default_rng(13)
    eng = _engine(lib)
    try:
        for kept, doubles in ((10, 0), (11, 1), (958, 1), (959, 0)):
            assert lib.sdv_needs_double_width(kept) == doubles
            for fmt in (ia.GRAY8, ia.YUYV422):
                want, doubled = ia.run_case(via, lib, eng, rng, fmt, kept + 3, 2, crop=(2, 1, 0, 0), double=ia.AUTO)
                assert doubled == doubles and want.shape == (1, 2, kept * (2 if doubles else 1))
    finally:
        lib.sdv_engine_destroy(eng)


def test_emu_auto_doubling(emu_lib):
    _auto_doubling(ia.emu(emu_lib), dc.HOST)


@pytest.mark.gpu
def test_gpu_auto_doubling():
    _auto_doubling(ia.product(), dc.DEVICE)


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------------
def _refusals(lib, via):
    """Host checks ahead of any launch: the code, a reason in sdv_last_error, the destination untouched, and a good call right behind.
    sdv_ingest_geometry gives the same code for the same descriptor."""
    rng = np.random.default_rng(17)
    eng = _engine(lib)
    w, h, n = 20, 6, 2
    rb = 2 * w
    s_span, d_span = n * h * rb, n * h * w
    raw = rng.integers(0, 256, size=4096, dtype=np.uint8)
    want, _ = ia.ingest_ref(raw, ia.UYVY422, w, h, n, rb, h * rb)
    src = via.array(raw)
    dst = via.array(np.full(4096, ia.FILL, dtype=np.uint8))
    sp, dp = via.ptr(src), via.ptr(dst)
    NULL = object()

    def call(d=None, s=sp, srs=rb, sfs=h * rb, frames=n, t=dp, drs=w, dfs=h * w, **kw):
        d = ia.desc(**dict(dict(fmt=ia.UYVY422, w=w, h=h), **kw)) if d is None else d
        return lib.sdv_ingest_frames(eng, None if d is NULL else C.byref(d), s, srs, sfs, frames, t, drs, dfs, via.stream())

    def refused(code, geo=False, **kw):
        assert call(**kw) == code, kw
        assert lib.sdv_last_error(eng), kw
        assert (via.get(dst) == ia.FILL).all(), kw
        if kw.get("d") is not NULL:         # the descriptor alone: refused for the same reason, or nothing wrong with it
            d = ia.desc(**dict(dict(fmt=ia.UYVY422, w=w, h=h), **{k: v for k, v in kw.items() if k in ("fmt", "w", "h", "crop", "colors", "double")}))
            assert lib.sdv_ingest_geometry(C.byref(d), None, None, None, None) == (code if geo else ia.OK), kw
        good = via.array(np.full(d_span + ia.TAIL, ia.FILL, dtype=np.uint8))            # ... and the engine takes the next call
        assert call(t=via.ptr(good)) == ia.OK
        got = via.get(good)
        assert np.array_equal(got[:d_span], want.reshape(-1)) and (got[d_span:] == ia.FILL).all()
    try:
        # null pointers
        refused(ia.BAD_ARG, d=NULL)
        assert lib.sdv_ingest_geometry(None, None, None, None, None) == ia.BAD_ARG
        refused(ia.NULL_VIDEO, s=None)
        refused(ia.NULL_PCM, t=None)
        # unknown enum values
        refused(ia.BAD_ARG, geo=True, fmt=9)
        refused(ia.BAD_ARG, geo=True, fmt=255)
        refused(ia.BAD_ARG, geo=True, colors=4)
        refused(ia.BAD_ARG, geo=True, double=3)
        # a colour channel from a format that has none
        for fmt in (ia.GRAY8, ia.UYVY422, ia.YUYV422, ia.V210, ia.GRAY10LE):
            for colors in (ia.R, ia.G, ia.B):
                refused(ia.UNSUPPORTED, geo=True, fmt=fmt, colors=colors)
        # crops that leave nothing, from each side; sizes that are none
        for crop in ((w, 0, 0, 0), (0, w, 0, 0), (w // 2, w // 2, 0, 0), (0, 0, h, 0), (0, 0, 0, h), (0, 0, h // 2, h // 2)):
            refused(ia.BAD_ARG, geo=True, crop=crop)
        refused(ia.BAD_ARG, geo=True, w=0)
        refused(ia.BAD_ARG, geo=True, h=0)
        refused(ia.BAD_ARG, geo=True, w=-5)
        refused(ia.BAD_ARG, geo=True, w=1, h=700, crop=(0, 0, 640, 0))          # (the forced bottom crop counts)
        # strides
        refused(ia.BAD_ARG, srs=rb - 1)
        refused(ia.BAD_ARG, sfs=h * rb - 1)
        refused(ia.BAD_ARG, drs=w - 1)
        refused(ia.BAD_ARG, dfs=h * w - 1)
        refused(ia.BAD_ARG, frames=-1)
        # overlap: the same pointer; the destination's first byte on the source's last one, and its last byte on the source's first one
        refused(ia.BAD_ARG, t=sp)
        refused(ia.BAD_ARG, s=dp + 1024, t=dp + 1024 + s_span - 1)
        refused(ia.BAD_ARG, s=dp + 1024, t=dp + 1024 - d_span + 1)
        # no frames ask nothing at all; one frame asks nothing of the frame strides
        assert call(frames=0, s=None, t=None, d=NULL) == ia.OK and (via.get(dst) == ia.FILL).all()
        assert call(frames=1, sfs=0, dfs=0, t=dp + 2048) == ia.OK
        got = via.get(dst)
        assert np.array_equal(got[2048:2048 + h * w], want[0].reshape(-1)) and (got[:2048] == ia.FILL).all() and (got[2048 + h * w:] == ia.FILL).all()
        # spans that touch do not overlap (source and destination in one buffer)
        both = via.array(np.concatenate([raw[:s_span], np.full(d_span + ia.TAIL, ia.FILL, dtype=np.uint8)]))
        assert call(s=via.ptr(both), t=via.ptr(both, s_span)) == ia.OK
        got = via.get(both)
        assert np.array_equal(got[:s_span], raw[:s_span]) and np.array_equal(got[s_span:s_span + d_span], want.reshape(-1)) and (got[s_span + d_span:] == ia.FILL).all()
    finally:
        lib.sdv_engine_destroy(eng)


def test_emu_refusals(emu_lib):
    _refusals(ia.emu(emu_lib), dc.HOST)


@pytest.mark.gpu
def test_gpu_refusals():
    _refusals(ia.product(), dc.DEVICE)


# ---- 6. what it makes decodes -----------------------------------------------------------------------------------------------------------------
BORDER = (5, 3, 2, 1)           # left, right, top, bottom


@functools.lru_cache(maxsize=None)
def _tape():
    """(the luma of a 717-pixel STC-007 tape, what the oracle makes of it doubled): made once for the six tests that read it"""
    luma, _, _ = synth.stc007_frames(n_frames=3, seed=51, width=717, height=48, noise_sigma=3.0)
    want, want_stats = oracle_binarize(np.repeat(luma, 2, axis=2), mode=2, doubled=True)
    luma.setflags(write=False)
    return luma, want.tobytes(), want_stats.tobytes()


def _feeds_the_decoder(lib, via, fmt_name, oracle_lib):
    """A tape inside a border of noise, packed with random chroma / low bits / alpha: ingest with the matching crop and DOUBLE_AUTO, then
    sdv_binarize_frames(NEW_FILE | DOUBLED): the records and frame descriptors the oracle makes of np.repeat(luma, 2)."""
    fmt = ia.FORMATS[fmt_name]
    luma, want, want_stats = _tape()
    rng = np.random.default_rng(19)
    n, h, w = luma.shape
    left, right, top, bottom = BORDER
    framed = rng.integers(0, 256, size=(n, top + h + bottom, left + w + right), dtype=np.uint8)
    framed[:, top:top + h, left:left + w] = luma
    eng = _engine(lib)
    try:
        plane, doubled = ia.run_case(via, lib, eng, rng, fmt, framed.shape[2], framed.shape[1], n=n, crop=BORDER, double=ia.AUTO,
                                     rows=ia.pack(fmt, framed, rng), src_pad=3, dst_pad=2)
        assert doubled == 1 and np.array_equal(plane, np.repeat(luma, 2, axis=2))
        lib.sdv_set_mode(eng, 2)
        # `plane` is the host array run_case has just proven equal, byte for byte, to what the call left in device memory; via.binarize uploads it
        # again.  The bytes are the same, but this is not the chain that stays in device memory from the capture buffer to the records:
        # test_gpu_engine_wrapper_feeds_the_decoder hands the device tensor on.
        rc, recs, stats = via.binarize(lib, eng, plane, first_frame_no=1, flags=1 | 2)
    finally:
        lib.sdv_engine_destroy(eng)
    assert rc == 0 and recs.tobytes() == want and stats.view(np.uint8).tobytes() == want_stats
    assert ((recs["flags"] & 64) != 0).sum() > 3 * 40


@pytest.mark.parametrize("fmt_name", ["uyvy422", "v210", "bgr0"])
def test_emu_feeds_the_decoder(fmt_name, emu_lib, oracle_lib):
    _feeds_the_decoder(ia.emu(emu_lib), dc.HOST, fmt_name, oracle_lib)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt_name", ["uyvy422", "v210", "bgr0"])
def test_gpu_feeds_the_decoder(fmt_name, oracle_lib):
    _feeds_the_decoder(ia.product(), dc.DEVICE, fmt_name, oracle_lib)


# ---- 7. the stream and the device of the call -------------------------------------------------------------------------------------------------
def _streamed_ingest(lib, device, A, B, geo):
    """Frame set A in the source buffer; on a busy non-blocking side stream of `device`: set B copied in, sdv_ingest_frames, the result cloned;
    that stream alone is waited for -> the result"""
    import torch
    fmt, w, h, n, srs, sfs, ow, oh = geo
    name = "cuda:%d" % device
    eng = C.c_void_p(lib.sdv_engine_create(device))
    assert eng, lib.sdv_last_error(None)
    side = torch.cuda.Stream(device=device)
    assert side.cuda_stream != 0
    src = torch.from_numpy(A.copy()).to(name)
    dst = torch.full((n * oh * ow,), ia.FILL, dtype=torch.uint8, device=name)
    ballast = torch.empty(256 << 20, dtype=torch.uint8, device=name)
    staged = torch.from_numpy(B.copy()).pin_memory()
    torch.cuda.synchronize(device)
    d = ia.desc(fmt, w, h)
    try:
        with torch.cuda.stream(side):
            for v in range(4):
                ballast.fill_(v)
            src.copy_(staged, non_blocking=True)
        rc = lib.sdv_ingest_frames(eng, C.byref(d), src.data_ptr(), srs, sfs, n, dst.data_ptr(), ow, oh * ow, C.c_void_p(side.cuda_stream))
        assert rc == 0, lib.sdv_last_error(eng)
        with torch.cuda.stream(side):
            out = dst.clone()
        side.synchronize()
        return out.cpu().numpy()
    finally:
        torch.cuda.synchronize(device)
        lib.sdv_engine_destroy(eng)


@pytest.mark.gpu
def test_gpu_ingest_runs_on_the_given_stream():
    """The call's work goes to the stream it is given: a launch on any other stream reads frame set A, or B half copied.  With two visible
    devices also: an engine of device 1 called while device 0 is current works on device 1 and leaves device 0 current."""
    import torch
    lib = ia.product()
    rng = np.random.default_rng(23)
    fmt, w, h, n = ia.UYVY422, 720, 64, 8
    rb = ia.row_bytes(fmt, w)
    A = rng.integers(0, 256, size=n * h * rb, dtype=np.uint8)
    B = rng.integers(0, 256, size=n * h * rb, dtype=np.uint8)
    want_a, _ = ia.ingest_ref(A, fmt, w, h, n, rb, h * rb)
    want_b, _ = ia.ingest_ref(B, fmt, w, h, n, rb, h * rb)
    assert not np.array_equal(want_a, want_b)
    geo = (fmt, w, h, n, rb, h * rb, w, h)
    assert np.array_equal(_streamed_ingest(lib, 0, A, B, geo), want_b.reshape(-1))
    if torch.cuda.device_count() >= 2:
        torch.cuda.set_device(0)
        got = _streamed_ingest(lib, 1, A, B, geo)
        assert torch.cuda.current_device() == 0
        assert np.array_equal(got, want_b.reshape(-1))
    else:
        print("one visible device: the device half of the contract was not run")


# ---- 8. the library ---------------------------------------------------------------------------------------------------------------------------
def test_symbols_of_the_product_library():
    from sdvpcmdecoder_amd import build as b
    lib = ia.bind(C.CDLL(b.build_hip()))
    assert hasattr(lib, "sdv_ingest_geometry") and hasattr(lib, "sdv_ingest_frames")
    assert lib.sdv_abi_version() >= 8
    assert C.sizeof(ia.Desc) == 20
    # the geometry needs neither an engine nor a device
    assert ia.geometry(lib, ia.desc(ia.V210, 720, 486, crop=(4, 6, 2, 4), double=ia.AUTO)) == (0, 1420, 480, 1, 1920)
    assert ia.geometry(lib, ia.desc(ia.RGB0, 1920, 1080)) == (0, 1920, 640, 0, 7680)


@pytest.mark.gpu
def test_gpu_engine_wrapper():
    """Engine.ingest / Engine.ingest_geometry: a (frames, rows, padded row bytes) tensor in, the plane and `doubled` out, on torch's current stream."""
    import torch
    from sdvpcmdecoder_amd import Engine, IngestDesc
    rng = np.random.default_rng(31)
    w, h, n, pad = 50, 7, 3, 112
    rb = ia.row_bytes(ia.V210, w)
    raw = rng.integers(0, 256, size=(n, h, rb + pad), dtype=np.uint8)
    eng = Engine(0)
    assert eng.ingest_geometry(IngestDesc(ia.V210, 0, ia.AUTO, 0, 3, 2, 1, 1, w, h)) == (90, 5, True, rb)
    got, doubled = eng.ingest(torch.from_numpy(raw).cuda(), "v210", w, h, crop=(3, 2, 1, 1))
    want, _ = ia.ingest_ref(raw.reshape(-1), ia.V210, w, h, n, rb + pad, h * (rb + pad), crop=(3, 2, 1, 1), double=ia.AUTO)
    assert doubled is True and got.shape == (n, 5, 90) and np.array_equal(got.cpu().numpy(), want)
    rgb = rng.integers(0, 256, size=(h, 3 * w), dtype=np.uint8)
    got, doubled = eng.ingest(torch.from_numpy(rgb).cuda(), ia.BGR24, w, h, colors=ia.R, double="off")
    assert doubled is False and np.array_equal(got.cpu().numpy()[0], rgb[:, 2::3])
    with pytest.raises(RuntimeError, match="colour channel"):
        eng.ingest(torch.from_numpy(raw).cuda(), "v210", w, h, colors=ia.G)


@pytest.mark.gpu
def test_gpu_engine_wrapper_feeds_the_decoder(oracle_lib):
    """The chain in device memory: Engine.ingest's tensor goes straight into Engine.binarize_frames(doubled=...), nothing comes back in between."""
    import torch
    from sdvpcmdecoder_amd import Engine
    luma, want, want_stats = _tape()
    rng = np.random.default_rng(37)
    n, h, w = luma.shape
    left, right, top, bottom = BORDER
    framed = rng.integers(0, 256, size=(n, top + h + bottom, left + w + right), dtype=np.uint8)
    framed[:, top:top + h, left:left + w] = luma
    eng = Engine(0)
    eng.setBinarizationMode(2)
    plane, doubled = eng.ingest(torch.from_numpy(ia.pack(ia.V210, framed, rng)).cuda(), "v210", framed.shape[2], framed.shape[1], crop=BORDER)
    recs, stats = eng.binarize_frames(plane, first_frame_no=1, new_file=True, doubled=doubled)
    torch.cuda.synchronize()
    assert doubled is True and recs.cpu().numpy().tobytes() == want and stats.cpu().numpy().tobytes() == want_stats


# ---- 9. from plain C++ ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_cpp_host_program_ingests(tmp_path):
    """decode_tape ingest: a v210 file with rows padded to 128 bytes, 2 frames of 50 x 6, crop 1,1,1,1 -> the plane of ingest_ref in a file and
    its geometry on stdout."""
    import subprocess
    from sdvpcmdecoder_amd import build as b
    exe = b.build_example()
    rng = np.random.default_rng(29)
    w, h, n = 50, 6, 2
    rb = ia.row_bytes(ia.V210, w)
    stride = (rb + 127) // 128 * 128
    assert rb == 144 and stride == 256
    raw = rng.integers(0, 256, size=n * h * stride, dtype=np.uint8)
    want, doubled = ia.ingest_ref(raw, ia.V210, w, h, n, stride, h * stride, crop=(1, 1, 1, 1), double=ia.AUTO)
    (tmp_path / "video.raw").write_bytes(raw.tobytes())
    out = subprocess.run([exe, "ingest", str(tmp_path / "video.raw"), "v210", str(w), str(h), str(stride), str(n), "1,1,1,1", "bw", "auto",
                          str(tmp_path / "luma.out")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr + out.stdout
    assert out.stdout.split() == ["96", "4", "1"] and want.shape == (n, 4, 96) and doubled == 1
    assert (tmp_path / "luma.out").read_bytes() == want.tobytes()
