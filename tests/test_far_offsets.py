"""Every entry that takes video promises "frame f, row r at base + f * frame_stride + r * row_stride" with strides of type size_t (include/sdvpcm.h).
Here those products leave 31 and 32 bits: frames 2 GiB apart (A), rows of one frame 32 MiB to 1 GiB apart (B), in sparse buffers of which only the
rows are ever written (tests/far_offsets.py has the layout, the tables and the lead-in that keeps a wrong kernel inside the allocation).  What is
expected never comes from the code under test: the oracle's records of the same frames held contiguously for the readers, the numpy references of
the header's text for the writers.  Every body is written once and handed host memory and the emulator build, or device memory and the product."""
import ctypes as C

import numpy as np
import pytest

import device_calls as dc
import far_offsets as fo
import geometry_cases as gc
from engine_api import STATS_DTYPE, launch_counts
from libs import LINE_DTYPE
from stitch_api import PAIR_DTYPE

FMT_NAMES = sorted(gc.FORMATS)
FUSED = [gc.STC007, gc.PCM1, gc.PCM16X0]
FUSED_IDS = ["stc007", "pcm1", "pcm16x0"]
STC_ROW_IDS = sorted(fo.STC_ROW_CASES)


def _engine(lib, mode=2, pcm_type=None):
    eng = C.c_void_p(lib.sdv_engine_create(0))
    gc.emu_configure(lib, eng, mode)
    if pcm_type is not None:
        lib.sdv_set_pcm_type(eng, pcm_type, 0)
        assert lib.sdv_set_pcm1_stitch_settings(eng, C.byref(gc.p1.default_settings())) == 0
        assert lib.sdv_set_pcm16x0_stitch_settings(eng, C.byref(gc.p16.default_settings())) == 0
    return eng


def _same(got, want):
    assert got.tobytes() == want.tobytes(), gc.first_difference(got, want)


# ---- the calls, on a layout ---------------------------------------------------------------------------------------------------------------------
def _frames_call(lib, via, eng, entry, rec_dtype, nrec, lay, first_frame_no=1, flags=0):
    """One frame call on the rows of `lay` -> (records, frame descriptors)"""
    recs, stats = via.zeros(nrec, rec_dtype), via.zeros(lay.n, STATS_DTYPE)
    rc = getattr(lib, entry)(eng, lay.address, lay.row_stride, lay.frame_stride, lay.w, lay.h, lay.n, first_frame_no, flags, via.ptr(recs), nrec,
                             via.ptr(stats), lay.n, via.stream())
    assert rc == 0, lib.sdv_last_error(eng)
    return via.get(recs), via.get(stats)


def _markerless_frames(lib, via, fmt_name, case, row_stride, frame_stride, mode):
    fmt = gc.FORMATS[fmt_name]
    frames, want, wstats = case
    n, h, _w = frames.shape
    lay = fo.sparse_frames(via is dc.DEVICE, frames, row_stride, frame_stride)
    eng = _engine(lib, mode)
    try:
        got, stats = _frames_call(lib, via, eng, fmt.frames_entry, fmt.rec_dtype, int(getattr(lib, fmt.count_fn)(h, n, 0)), lay)
    finally:
        lib.sdv_engine_destroy(eng)
        lay.release()
    _same(got, want)
    _same(stats, wstats)


def _decode(lib, via, pcm_type, want, row_stride, frame_stride):
    from test_decode_frames import FRASM
    frames, want_p, want_f, want_s = want
    n, h, w = frames.shape
    lay = fo.sparse_frames(via is dc.DEVICE, frames, row_stride, frame_stride)
    eng = _engine(lib, 2, pcm_type)
    try:
        cap, fcap, nst = (n + 2) * 1800 + 8192, n + 16, n + 1
        pairs, fr, stats = via.zeros(cap, PAIR_DTYPE), via.zeros(fcap, FRASM[pcm_type]), via.zeros(nst, STATS_DTYPE)
        npairs, nfr, npur, nm = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_uint64(0)
        rc = lib.sdv_decode_frames(eng, pcm_type, lay.address, row_stride, lay.frame_stride, w, h, n, 1, 1 | 4, via.ptr(pairs), cap, C.byref(npairs),
                                   via.ptr(fr), fcap, C.byref(nfr), via.ptr(stats), nst, 0, 0, None, 0, C.byref(npur), C.byref(nm), via.stream())
        assert rc == 0, lib.sdv_last_error(eng)
        got_p, got_f, got_s = via.get(pairs, npairs.value), via.get(fr, nfr.value), via.get(stats)
    finally:
        lib.sdv_engine_destroy(eng)
        lay.release()
    _same(got_p, want_p)
    _same(got_f, want_f)
    assert got_s.view(np.uint8).tobytes() == want_s.tobytes()


# ---- A: ordinary rows, frames far apart ------------------------------------------------------------------------------------------------------------
def _frames_far_apart(fmt_name, lib, via):
    case = fo.frame_case(fmt_name)
    _markerless_frames(lib, via, fmt_name, case, case[0].shape[2] + fo.ROW_PAD, fo.FAR_FRAME_STRIDE, 2)


def _stc007_frames_far_apart(tape, lib, via):
    """The clean tape: the lean kernel alone.  The worn one: the lean, the general and the five-wave kernel, and the sweep kernels."""
    luma, want, wstats, split = fo.stc_frame_case(tape)
    counts = _stc007_behind_a_cold_frame(lib, via, luma, want, wstats, split, luma.shape[2] + fo.ROW_PAD, fo.FAR_FRAME_STRIDE)
    general = None if counts is None else counts["snap_frames"] + counts["plain_frames"]
    if counts is not None and tape == "worn":
        assert counts["lean_frames"] >= 3 and general > 0 and counts["fat_frames"] > 0 and counts["sweep_levels_reqs"] > 0 and counts["sweep_pick_reqs"] > 0, counts
    if counts is not None and tape == "clean":
        assert counts["lean_frames"] == 3 and general + counts["fat_frames"] == 0, counts


def _decode_frames_far_apart(pcm_type, lib, via):
    want = fo.chain_case(pcm_type, "frames")
    _decode(lib, via, pcm_type, want, want[0].shape[2] + fo.ROW_PAD, fo.FAR_FRAME_STRIDE)


# ---- B: rows far apart inside a frame -----------------------------------------------------------------------------------------------------------------
def _rows_far_apart(fmt_name, lib, via):
    _kw, mode, row_stride, _run = fo.ROW_CASES[fmt_name]
    _markerless_frames(lib, via, fmt_name, fo.row_case(fmt_name), row_stride, None, mode)


def _stc007_behind_a_cold_frame(lib, via, luma, want, wstats, split, row_stride, frame_stride):
    """The first frame from an ordinary buffer (NEW_FILE: the cold frame), the others in one call from the sparse layout; the records and descriptors
    of both calls against the oracle's.  -> the launch counts of the second call, where the build has them (developer builds), or None"""
    n, h, w = luma.shape
    lay = fo.sparse_frames(via is dc.DEVICE, luma[1:], row_stride, frame_stride)
    eng = _engine(lib)
    try:
        first = via.array(luma[:1])
        recs, stats = via.zeros(split, LINE_DTYPE), via.zeros(1, STATS_DTYPE)
        rc = lib.sdv_binarize_frames(eng, via.ptr(first), w, w * h, w, h, 1, 1, 1, via.ptr(recs), split, via.ptr(stats), 1, via.stream())
        assert rc == 0, lib.sdv_last_error(eng)
        got0, stats0 = via.get(recs), via.get(stats)
        got1, stats1 = _frames_call(lib, via, eng, "sdv_binarize_frames", LINE_DTYPE, (n - 1) * (h + 3), lay, first_frame_no=2)
        counts = launch_counts(lib, eng) if hasattr(lib, "sdv_dev_launch_counts") else None
    finally:
        lib.sdv_engine_destroy(eng)
        lay.release()
    _same(np.concatenate([got0, got1]), want)
    _same(np.concatenate([stats0, stats1]), wstats)
    return counts


def _stc007_rows_far_apart(name, lib, via):
    """The second frame of a tape that plays - the lean kernel's - from rows far apart."""
    height, row_stride, captured, _beyond = fo.STC_ROW_CASES[name]
    counts = _stc007_behind_a_cold_frame(lib, via, *fo.stc_row_case(height), row_stride, None)
    if counts is not None and captured:
        general = counts["snap_frames"] + counts["plain_frames"] + counts["fat_frames"]
        assert counts["lean_frames"] == 1 and general == 0, "the frame was meant for the lean build alone: %s" % counts


def _lines_far_apart(name, lib, via):
    """The rows of the B cases as lines of their own, one row per line, nothing preset."""
    if name == "stc007":
        rows, want = fo.stc_lines_case()
        row_stride, fmt, k, wscans = fo.STC_ROW_CASES["rows_beyond_4g"][1], None, 1, None
    else:
        rows, want, wscans = fo.row_lines_case(name)
        row_stride, fmt = fo.ROW_CASES[name][2], gc.FORMATS[name]
        k = fmt.recs_per_line
    n, w = rows.shape
    lay = fo.sparse_frames(via is dc.DEVICE, rows[None], row_stride)
    eng = _engine(lib, 2 if fmt is None else fo.ROW_CASES[name][1])
    try:
        recs = via.zeros(k * n, LINE_DTYPE if fmt is None else fmt.rec_dtype)
        scans = via.zeros(k * n, np.uint8) if k == 3 else None
        if fmt is None:
            rc = lib.sdv_binarize_lines(eng, lay.address, row_stride, w, n, None, 1, 1, 1, 0, via.ptr(recs), n, via.stream())
        else:
            args = [eng, lay.address, row_stride, w, n, None, 1, 1, 1, 0, 1, via.ptr(recs), k * n] + ([via.ptr(scans)] if k == 3 else []) + [via.stream()]
            rc = getattr(lib, fmt.lines_entry)(*args)
        assert rc == 0, lib.sdv_last_error(eng)
        got = via.get(recs)
        got_scans = via.get(scans) if k == 3 else None
    finally:
        lib.sdv_engine_destroy(eng)
        lay.release()
    _same(got, want)
    if wscans is not None:
        assert (got_scans == wscans).all()


def _decode_rows_far_apart(lib, via):
    _decode(lib, via, gc.PCM1, fo.chain_case(gc.PCM1, "rows"), fo.ROW_CASES["pcm1"][2], None)


# ---- the writers: far frames (two, 2^32 apart) and far rows (five, 2^30 + 16 apart) ------------------------------------------------------------------
def _near(via, n, h, row_bytes, rows=None):
    """An ordinary buffer of n * h rows, FILL or `rows`, with EDGE bytes of FILL behind them -> (buffer, row_stride, frame_stride)"""
    flat = np.full(n * h * row_bytes + fo.EDGE, fo.FILL, dtype=np.uint8)
    if rows is not None:
        flat[:n * h * row_bytes] = np.ascontiguousarray(rows).reshape(-1)
    return via.array(flat), row_bytes, h * row_bytes


def _near_rows(via, buf, n, h, row_bytes):
    """-> (the rows of a _near buffer, whether what lies behind them still holds FILL)"""
    got = via.get(buf)
    return got[:n * h * row_bytes].reshape(n, h, row_bytes), bool((got[n * h * row_bytes:] == fo.FILL).all())


def _written(lay, want):
    got = lay.rows()
    clean = lay.rest_untouched()
    assert np.array_equal(got, want), "(frame, row) that differ: %s" % np.argwhere((got != want).any(axis=2)).tolist()
    assert clean, "bytes outside the destination rows were written"


def _encoder_far(name, term, lib, via):
    import encode_packed_api as ep
    n, h, _, _ = fo.writer_geometry(term, 0)
    d, pcm, want = fo.encoder_case(name, n, h)
    _, _, row_stride, frame_stride = fo.writer_geometry(term, want.shape[2])
    lay = fo.Sparse(via is dc.DEVICE, n, h, want.shape[2], row_stride, frame_stride)
    eng = C.c_void_p(lib.sdv_engine_create(0))
    try:
        src = via.array(pcm.reshape(-1))
        rc = ep.frames_call(lib, d)(eng, C.byref(d), via.ptr(src), len(pcm), n, lay.address, row_stride, frame_stride, via.stream())
        assert rc == 0, lib.sdv_last_error(eng)
        _written(lay, want)
    finally:
        lib.sdv_engine_destroy(eng)
        lay.release()


def _ingest_far(side, term, lib, via):
    """side: which of the two buffers is the far one; the other is an ordinary buffer (the two spans must not overlap, and one far layout is held at a time)"""
    import ingest_api as ia
    n, h, _, _ = fo.writer_geometry(term, 0)
    rows, want = fo.ingest_case(n, h)
    rb, w = rows.shape[2], want.shape[2]
    d = ia.desc(ia.UYVY422, w, h)
    eng = C.c_void_p(lib.sdv_engine_create(0))
    lay = None
    try:
        if side == "source":
            _, _, srs, sfs = fo.writer_geometry(term, rb)
            lay = fo.Sparse(via is dc.DEVICE, n, h, rb, srs, sfs).put(rows)
            dst, drs, dfs = _near(via, n, h, w)
            rc = lib.sdv_ingest_frames(eng, C.byref(d), lay.address, srs, sfs, n, via.ptr(dst), drs, dfs, via.stream())
            assert rc == 0, lib.sdv_last_error(eng)
            got, clean = _near_rows(via, dst, n, h, w)
            assert np.array_equal(got, want) and clean
            assert np.array_equal(lay.rows(), rows)             # the source is read only
        else:
            _, _, drs, dfs = fo.writer_geometry(term, w)
            lay = fo.Sparse(via is dc.DEVICE, n, h, w, drs, dfs)
            src, srs, sfs = _near(via, n, h, rb, rows)
            rc = lib.sdv_ingest_frames(eng, C.byref(d), via.ptr(src), srs, sfs, n, lay.address, drs, dfs, via.stream())
            assert rc == 0, lib.sdv_last_error(eng)
            _written(lay, want)
    finally:
        lib.sdv_engine_destroy(eng)
        if lay is not None:
            lay.release()


def _double_width_far(side, lib, via):
    n, h, row_stride, _ = fo.writer_geometry("rows", 0)
    rows = np.random.default_rng(41).integers(0, 256, size=(1, h, fo.WRITER_WIDTH), dtype=np.uint8)
    want = np.repeat(rows, 2, axis=2)
    w = fo.WRITER_WIDTH
    eng = C.c_void_p(lib.sdv_engine_create(0))
    lay = None
    try:
        if side == "source":
            lay = fo.Sparse(via is dc.DEVICE, 1, h, w, row_stride, 0).put(rows)
            dst, drs, _ = _near(via, 1, h, 2 * w)
            rc = lib.sdv_double_width(eng, lay.address, row_stride, w, h, via.ptr(dst), drs, via.stream())
            assert rc == 0, lib.sdv_last_error(eng)
            got, clean = _near_rows(via, dst, 1, h, 2 * w)
            assert np.array_equal(got, want) and clean
        else:
            lay = fo.Sparse(via is dc.DEVICE, 1, h, 2 * w, row_stride, 0)
            src, srs, _ = _near(via, 1, h, w, rows)
            rc = lib.sdv_double_width(eng, via.ptr(src), srs, w, h, lay.address, row_stride, via.stream())
            assert rc == 0, lib.sdv_last_error(eng)
            _written(lay, want)
    finally:
        lib.sdv_engine_destroy(eng)
        if lay is not None:
            lay.release()


# ---- C: the row cases can tell ----------------------------------------------------------------------------------------------------------------------
def test_the_row_cases_can_tell_a_cut_offset():
    """A row case chosen at random passes on code that forms its offsets in 32 bits (far_offsets.aliases says why).  Every case whose rows leave 32
    bits has, within the longest run of its capture loop, a line whose cut offset is the true offset of another line; the two STC-007 cases on
    either side of the capture's guard keep every offset below 2^31 - they pin which side takes the capture - and say so."""
    for name, (kw, _mode, row_stride, run) in fo.ROW_CASES.items():
        assert fo.can_tell(row_stride, kw["height"], run), name
    for name, (height, row_stride, captured, beyond) in fo.STC_ROW_CASES.items():
        assert captured == (row_stride * height < 1 << 31), name
        assert beyond == ((height - 1) * row_stride >= 1 << 32), name
        if beyond:
            assert fo.can_tell(row_stride, height, fo.STC007_RUN, starts=(0,)), name
        else:
            assert (height - 1) * row_stride + 720 <= 1 << 31 and not fo.aliases(row_stride, height, fo.STC007_RUN, starts=(0,)), name
    # ... and the strides that pass on the defective code do so because nothing aliases: 36 MiB rows of PCM-1
    assert not fo.can_tell(36 << 20, 72, fo.PCM1_RUN) and not fo.aliases(36 << 20, 72, fo.PCM1_RUN)


def test_the_row_cases_read(oracle_lib):
    """An aliased line shows only if it reads: in the oracle's run every data line of the row cases has a valid CRC but, at most, the first of a field."""
    from sdvpcmdecoder_amd.abi import LF_CRC_VALID
    for name in FMT_NAMES:
        _, recs, _ = fo.row_case(name)
        data = recs[recs["service_type"] == 0]
        assert ((data["flags"] & LF_CRC_VALID) != 0).sum() >= len(data) - 2 * gc.FORMATS[name].recs_per_line, name
    for height in (64, 66):
        _, recs, _, split = fo.stc_row_case(height)
        data = recs[split:][recs[split:]["service_type"] == 0]
        assert (data["calc_crc"] == data["words"][:, 8]).all(), height


def test_the_sparse_layout_sees_a_stray_write():
    """The host side of far_offsets.Sparse on a small and on a far layout: rows come back, a byte beside a row or where a row's cut or sign-extended
    offset lands fails rest_untouched, a byte in a row does not."""
    rng = np.random.default_rng(5)
    for rs, n_rows in ((64, 5), (fo.WRITER_ROW_STRIDE, fo.WRITER_ROWS)):
        rows = rng.integers(0, 256, size=(1, n_rows, 48), dtype=np.uint8)
        far = rs > 64
        for stray in (None, "in_row", "beside", "cut", "signed"):
            if stray in ("cut", "signed") and not far:
                continue
            lay = fo.sparse_frames(False, rows, rs)
            assert lay.lead >= (fo.LEAD if far else fo.SMALL_LEAD) and np.array_equal(lay.rows(), rows)
            o = lay.offsets[4]
            at = {None: None, "in_row": o + 3, "beside": o + 48 + 5, "cut": fo.cut32(o) + 7, "signed": fo.sign32(lay.offsets[2]) + 7}[stray]
            if at is not None:
                lay.buf[lay.lead + at] ^= 0xFF
            assert lay.rest_untouched() == (stray in (None, "in_row")), (rs, stray)
            lay.release()


# ---- the twins --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt_name", FMT_NAMES)
def test_emu_frames_far_apart(fmt_name, emu_lib, oracle_lib):
    _frames_far_apart(fmt_name, dc.emu_lib_of(emu_lib), dc.HOST)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt_name", FMT_NAMES)
def test_gpu_frames_far_apart(fmt_name, oracle_lib):
    _frames_far_apart(fmt_name, dc.product_lib(), dc.DEVICE)


@pytest.mark.parametrize("tape", ["clean", "worn"])
def test_emu_stc007_frames_far_apart(tape, emu_lib, oracle_lib):
    _stc007_frames_far_apart(tape, dc.emu_lib_of(emu_lib), dc.HOST)


@pytest.mark.gpu
@pytest.mark.parametrize("tape", ["clean", "worn"])
def test_gpu_stc007_frames_far_apart(tape, oracle_lib):
    _stc007_frames_far_apart(tape, dc.product_lib(), dc.DEVICE)


@pytest.mark.parametrize("pcm_type", FUSED, ids=FUSED_IDS)
def test_emu_decode_frames_far_apart(pcm_type, emu_lib, oracle_lib):
    _decode_frames_far_apart(pcm_type, dc.emu_lib_of(emu_lib), dc.HOST)


@pytest.mark.gpu
@pytest.mark.parametrize("pcm_type", FUSED, ids=FUSED_IDS)
def test_gpu_decode_frames_far_apart(pcm_type, oracle_lib):
    _decode_frames_far_apart(pcm_type, dc.product_lib(), dc.DEVICE)


@pytest.mark.parametrize("fmt_name", FMT_NAMES)
def test_emu_rows_far_apart(fmt_name, emu_lib, oracle_lib):
    _rows_far_apart(fmt_name, dc.emu_lib_of(emu_lib), dc.HOST)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt_name", FMT_NAMES)
def test_gpu_rows_far_apart(fmt_name, oracle_lib):
    _rows_far_apart(fmt_name, dc.product_lib(), dc.DEVICE)


@pytest.mark.parametrize("name", STC_ROW_IDS)
def test_emu_stc007_rows_far_apart(name, emu_lib, oracle_lib):
    _stc007_rows_far_apart(name, dc.emu_lib_of(emu_lib), dc.HOST)


@pytest.mark.gpu
@pytest.mark.parametrize("name", STC_ROW_IDS)
def test_gpu_stc007_rows_far_apart(name, oracle_lib):
    _stc007_rows_far_apart(name, dc.product_lib(), dc.DEVICE)


@pytest.mark.parametrize("name", FMT_NAMES + ["stc007"])
def test_emu_lines_far_apart(name, emu_lib, oracle_lib):
    _lines_far_apart(name, dc.emu_lib_of(emu_lib), dc.HOST)


@pytest.mark.gpu
@pytest.mark.parametrize("name", FMT_NAMES + ["stc007"])
def test_gpu_lines_far_apart(name, oracle_lib):
    _lines_far_apart(name, dc.product_lib(), dc.DEVICE)


def test_emu_decode_rows_far_apart(emu_lib, oracle_lib):
    _decode_rows_far_apart(dc.emu_lib_of(emu_lib), dc.HOST)


@pytest.mark.gpu
def test_gpu_decode_rows_far_apart(oracle_lib):
    _decode_rows_far_apart(dc.product_lib(), dc.DEVICE)


@pytest.mark.parametrize("term", ["frames", "rows"])
@pytest.mark.parametrize("name", sorted(fo.ENCODERS))
def test_emu_encoders_write_far_apart(name, term, emu_lib):
    _encoder_far(name, term, dc.emu_lib_of(emu_lib), dc.HOST)


@pytest.mark.gpu
@pytest.mark.parametrize("term", ["frames", "rows"])
@pytest.mark.parametrize("name", sorted(fo.ENCODERS))
def test_gpu_encoders_write_far_apart(name, term):
    _encoder_far(name, term, dc.product_lib(), dc.DEVICE)


@pytest.mark.parametrize("term", ["frames", "rows"])
@pytest.mark.parametrize("side", ["source", "destination"])
def test_emu_ingest_far_apart(side, term, emu_lib):
    _ingest_far(side, term, dc.emu_lib_of(emu_lib), dc.HOST)


@pytest.mark.gpu
@pytest.mark.parametrize("term", ["frames", "rows"])
@pytest.mark.parametrize("side", ["source", "destination"])
def test_gpu_ingest_far_apart(side, term):
    _ingest_far(side, term, dc.product_lib(), dc.DEVICE)


@pytest.mark.parametrize("side", ["source", "destination"])
def test_emu_double_width_far_apart(side, emu_lib):
    _double_width_far(side, dc.emu_lib_of(emu_lib), dc.HOST)


@pytest.mark.gpu
@pytest.mark.parametrize("side", ["source", "destination"])
def test_gpu_double_width_far_apart(side):
    _double_width_far(side, dc.product_lib(), dc.DEVICE)
