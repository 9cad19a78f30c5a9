"""The front halves of PCM-1 and PCM-16x0 on frames and lines that are not contiguous, aligned and even: padded rows, frames with gaps between them or
none at all, a start that is not 16-byte aligned, widths that are no multiple of 16 up to the widest the entry points take, odd heights, frames too short
for the prescan (tests/geometry_cases.py has the tables and says what each row reaches).  The reference is the oracle on the contiguous copy of the same
pixels; records, frame descriptors and scan_done marks are compared bytewise.  The outputs are the caller's, with guard records behind what the call may
write.  Every case runs on the SIMT emulator (CPU) and - gpu-marked - through Engine on the GPU."""
import ctypes as C

import numpy as np
import pytest

import geometry_cases as gc
from sdvpcmdecoder_amd.abi import LF_CRC_VALID, LF_BY_EXT_TUNE

FMT_NAMES = sorted(gc.FORMATS)
FRAME_IDS = [gc.shape_id(s) for s in gc.FRAME_SHAPES]
LINE_IDS = [gc.shape_id(s) for s in gc.LINE_SHAPES]
FUSED = [gc.STC007, gc.PCM1, gc.PCM16X0]
FUSED_IDS = ["stc007", "pcm1", "pcm16x0"]


def _placed_frames(fmt_name, idx):
    frames, want, wstats = gc.frames_case(fmt_name, idx)
    w, h, pad, shift, gap, mode = gc.FRAME_SHAPES[idx]
    beside = gc.make_frames(gc.FORMATS[fmt_name], w, h, seed=800 + idx) if pad == w else None
    return gc.place(frames, pad, shift, gap, seed=1000 + idx, beside=beside), want, wstats, mode


def _placed_stream(fmt_name):
    frames, want, wstats = gc.stream_case(fmt_name)
    _w, _h, pad, shift, gap, mode = gc.FRAME_SHAPES[gc.STREAM_SHAPE]
    return gc.place(frames, pad, shift, gap, seed=1050), want, wstats, mode


def _placed_lines(fmt_name, idx):
    block, step, runs = gc.lines_case(fmt_name, idx)
    _w, pad, shift, _how, mode = gc.LINE_SHAPES[idx]
    return gc.place(block, pad, shift, 0, seed=1070 + idx), step, runs, mode


def _check_frames(got, stats, nrec, n, want, wstats):
    assert gc.guards_intact(got, nrec), "a record behind the %d the call may write was written" % nrec
    assert gc.guards_intact(stats, n), "a frame descriptor behind the %d the call may write was written" % n
    assert got[:nrec].tobytes() == want.tobytes(), gc.first_difference(got[:nrec], want)
    assert stats[:n].tobytes() == wstats.tobytes(), gc.first_difference(stats[:n], wstats)


def _check_lines(got, scans, want, wscans):
    assert gc.guards_intact(got, len(want)), "a record behind the %d the call may write was written" % len(want)
    assert got[:len(want)].tobytes() == want.tobytes(), gc.first_difference(got[:len(want)], want)
    if wscans is not None:
        assert gc.guards_intact(scans, len(wscans)) and (scans[:len(wscans)] == wscans).all()


def _check_fused(pairs, n_pairs, frames, n_fr, stats, nst, want):
    _, want_p, want_f, want_s = want
    assert gc.guards_intact(pairs, n_pairs) and gc.guards_intact(frames, n_fr) and gc.guards_intact(stats, nst)
    assert n_pairs == len(want_p) and pairs[:n_pairs].tobytes() == want_p.tobytes()
    assert n_fr == len(want_f) and frames[:n_fr].tobytes() == want_f.tobytes()
    assert stats[:nst].tobytes() == want_s.tobytes()


# ---- the tables themselves -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt_name", FMT_NAMES)
def test_the_frames_of_the_tables_read(fmt_name, oracle_lib):
    """A table whose lines nobody can read would compare empty records.  In the oracle's run every data line of every shape has a valid CRC but, at
    most, the first line of each field (the worker does not trust it); the streamed tape has lost lines; the line cases read cold (PCM-16x0: the pass
    that searches the coordinates) and, preset from the neighbour, most of them read with what they were given."""
    k = gc.FORMATS[fmt_name].recs_per_line
    for idx, (w, h, *_rest) in enumerate(gc.FRAME_SHAPES):
        _, recs, _ = gc.frames_case(fmt_name, idx)
        data = recs[recs["service_type"] == 0]
        assert ((data["flags"] & LF_CRC_VALID) != 0).sum() >= len(data) - 2 * gc.N_FRAMES * k, (w, h)
    _, recs, _ = gc.stream_case(fmt_name)
    data = recs[recs["service_type"] == 0]
    valid = ((data["flags"] & LF_CRC_VALID) != 0).mean()
    assert 0.5 < valid < 0.97, valid
    for idx in range(len(gc.LINE_SHAPES)):
        _, _, ((_, cold, _), (_, warm, _)) = gc.lines_case(fmt_name, idx)
        assert ((cold["flags"][::k] & LF_CRC_VALID) != 0).all(), idx
        assert ((warm["flags"] & LF_CRC_VALID) != 0).all() and ((warm["flags"] & LF_BY_EXT_TUNE) != 0).sum() * 2 > len(warm), idx


# ---- the kernels on the emulator ---------------------------------------------------------------------------------------------------------------
def _emu_engine(lib, mode):
    eng = C.c_void_p(lib.sdv_engine_create(0))
    gc.emu_configure(lib, eng, mode)
    return eng


@pytest.mark.parametrize("idx", range(len(gc.FRAME_SHAPES)), ids=FRAME_IDS)
@pytest.mark.parametrize("fmt_name", FMT_NAMES)
def test_emu_frames_in_awkward_buffers(fmt_name, idx, emu_lib, oracle_lib):
    placed, want, wstats, mode = _placed_frames(fmt_name, idx)
    eng = _emu_engine(emu_lib, mode)
    rc, got, stats, nrec = gc.emu_frames(emu_lib, eng, gc.FORMATS[fmt_name], placed)
    err = emu_lib.sdv_last_error(eng)
    info = gc.ea.RunInfo()
    emu_lib.sdv_get_run_info(eng, C.byref(info))
    emu_lib.sdv_engine_destroy(eng)
    assert rc == 0, err
    _check_frames(got, stats, nrec, gc.N_FRAMES, want, wstats)
    if gc.lean_build_alone(gc.FRAME_SHAPES[idx]):
        assert info.frames_general == 0, "the lean build gave %d frames of a tape that plays to the full build" % info.frames_general


@pytest.mark.parametrize("fmt_name", FMT_NAMES)
def test_emu_stream_in_awkward_buffers(fmt_name, emu_lib, oracle_lib):
    """12 damaged frames of 717 x 25 in calls of 1, 7 and 4: the chain state crosses the calls, the repair rounds read the rows again through the same strides."""
    placed, want, wstats, mode = _placed_stream(fmt_name)
    fmt = gc.FORMATS[fmt_name]
    eng = _emu_engine(emu_lib, mode)
    got, gst, at = [], [], 0
    for cnt in gc.STREAM_CALLS:
        rc, recs, stats, nrec = gc.emu_frames(emu_lib, eng, fmt, placed, first_frame=at, n=cnt, first_frame_no=1 + at, new_file=(at == 0))
        assert rc == 0, emu_lib.sdv_last_error(eng)
        assert gc.guards_intact(recs, nrec) and gc.guards_intact(stats, cnt)
        got.append(recs[:nrec]); gst.append(stats[:cnt])
        at += cnt
    emu_lib.sdv_engine_destroy(eng)
    got, gst = np.concatenate(got), np.concatenate(gst)
    assert got.tobytes() == want.tobytes(), gc.first_difference(got, want)
    assert gst.tobytes() == wstats.tobytes(), gc.first_difference(gst, wstats)


@pytest.mark.parametrize("idx", range(len(gc.LINE_SHAPES)), ids=LINE_IDS)
@pytest.mark.parametrize("fmt_name", FMT_NAMES)
def test_emu_lines_in_awkward_buffers(fmt_name, idx, emu_lib, oracle_lib):
    placed, step, runs, mode = _placed_lines(fmt_name, idx)
    fmt = gc.FORMATS[fmt_name]
    _, n_rows, w = placed.shape
    eng = _emu_engine(emu_lib, mode)
    for states, want, wscans in runs:
        rc, got, scans = gc.emu_lines_raw(emu_lib, eng, fmt, placed.ptr(), step * placed.row_stride, w, n_rows // step, states)
        assert rc == 0, emu_lib.sdv_last_error(eng)
        _check_lines(got, scans, want, wscans)
    emu_lib.sdv_engine_destroy(eng)


@pytest.mark.parametrize("pcm_type", FUSED, ids=FUSED_IDS)
def test_emu_fused_call_in_an_awkward_buffer(pcm_type, emu_lib, oracle_lib):
    want = gc.fused_case(pcm_type)
    placed = gc.place(want[0], gc.FUSED_PAD, gc.FUSED_SHIFT, 0, seed=1090 + pcm_type)
    eng = _emu_engine(emu_lib, 2)
    emu_lib.sdv_set_pcm_type(eng, pcm_type, 0)
    assert emu_lib.sdv_set_pcm1_stitch_settings(eng, C.byref(gc.p1.default_settings())) == 0
    assert emu_lib.sdv_set_pcm16x0_stitch_settings(eng, C.byref(gc.p16.default_settings())) == 0
    rc, pairs, n_pairs, frames, n_fr, stats, nst = gc.emu_decode(emu_lib, eng, pcm_type, placed)
    err = emu_lib.sdv_last_error(eng)
    emu_lib.sdv_engine_destroy(eng)
    assert rc == 0, err
    _check_fused(pairs, n_pairs, frames, n_fr, stats, nst, want)


def test_emu_refuses_geometry_it_cannot_take(emu_lib):
    """row_stride < width, a line wider than the staged row, frames that overlap: SDV_ERR_BAD_ARG, and nothing written."""
    h, w = 8, 720
    luma = np.zeros(2 * h * (gc.PX_BYTES + 1) + 64, dtype=np.uint8)
    eng = _emu_engine(emu_lib, 2)
    for fmt in gc.FORMATS.values():
        for rs, fs, ww, n in ((w - 1, h * w, w, 1), (gc.PX_BYTES + 1, h * (gc.PX_BYTES + 1), gc.PX_BYTES + 1, 1), (w + 3, (h - 1) * (w + 3) + w - 1, w, 2)):
            rc, recs, stats, _ = gc.emu_frames_raw(emu_lib, eng, fmt, luma.ctypes.data, rs, fs, ww, h, n)
            assert rc == gc.BAD_ARG and gc.guards_intact(recs, 0) and gc.guards_intact(stats, 0), (fmt.name, rs, fs, ww, n)
        for rs, ww in ((w - 1, w), (gc.PX_BYTES + 1, gc.PX_BYTES + 1)):
            rc, recs, scans = gc.emu_lines_raw(emu_lib, eng, fmt, luma.ctypes.data, rs, ww, 4, None)
            assert rc == gc.BAD_ARG and gc.guards_intact(recs, 0) and (scans is None or gc.guards_intact(scans, 0)), (fmt.name, rs, ww)
        # ... and the tightest frame_stride that is legal is taken
        rc, _, _, _ = gc.emu_frames_raw(emu_lib, eng, fmt, luma.ctypes.data, w + 3, (h - 1) * (w + 3) + w, w, h, 2)
        assert rc == 0, emu_lib.sdv_last_error(eng)
    emu_lib.sdv_engine_destroy(eng)


# ---- the product on the GPU, through Engine --------------------------------------------------------------------------------------------------------
def _gpu_engine(mode):
    import torch
    torch.zeros(1, device="cuda:0")         # torch first: it brings up the HIP runtime it ships before the library's own first HIP call
    from sdvpcmdecoder_amd import Engine
    eng = Engine(0)
    eng.setBinarizationMode(mode)
    return eng, torch


def _gpu_guarded(torch, count, rec_bytes):
    return torch.full((count, rec_bytes), gc.GUARD, dtype=torch.uint8, device="cuda:0")


def _gpu_frames(eng, torch, fmt, view, first_frame_no=1, new_file=False):
    """One frame call; the outputs two records and one descriptor longer than the slices the call is given.  -> (records, descriptors, count) on the host"""
    n, h, _w = view.shape
    nrec = int(getattr(eng.lib, fmt.count_fn)(h, n, 1 if new_file else 0))
    lines, stats = _gpu_guarded(torch, nrec + 2, fmt.rec_dtype.itemsize), _gpu_guarded(torch, n + 1, 32)
    call = eng.pcm1_binarize_frames if fmt.name == "pcm1" else eng.pcm16x0_binarize_frames
    call(view, first_frame_no=first_frame_no, new_file=new_file, out_lines=lines[:nrec], out_stats=stats[:n])
    torch.cuda.synchronize()
    return lines.cpu().numpy().reshape(-1).view(fmt.rec_dtype), stats.cpu().numpy().reshape(-1).view(gc.ea.STATS_DTYPE), nrec


@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(len(gc.FRAME_SHAPES)), ids=FRAME_IDS)
@pytest.mark.parametrize("fmt_name", FMT_NAMES)
def test_gpu_frames_in_awkward_buffers(fmt_name, idx, oracle_lib):
    placed, want, wstats, mode = _placed_frames(fmt_name, idx)
    eng, torch = _gpu_engine(mode)
    view = placed.torch_view(torch)
    assert view.stride(1) == placed.row_stride and view.stride(0) == placed.frame_stride and view.data_ptr() % 16 == placed.start % 16
    got, stats, nrec = _gpu_frames(eng, torch, gc.FORMATS[fmt_name], view)
    info = eng.run_info()
    eng.close()
    _check_frames(got, stats, nrec, gc.N_FRAMES, want, wstats)
    if gc.lean_build_alone(gc.FRAME_SHAPES[idx]):
        assert info.frames_general == 0, "the lean build gave %d frames of a tape that plays to the full build" % info.frames_general


@pytest.mark.gpu
@pytest.mark.parametrize("fmt_name", FMT_NAMES)
def test_gpu_stream_in_awkward_buffers(fmt_name, oracle_lib):
    placed, want, wstats, mode = _placed_stream(fmt_name)
    fmt = gc.FORMATS[fmt_name]
    eng, torch = _gpu_engine(mode)
    got, gst, at = [], [], 0
    for cnt in gc.STREAM_CALLS:
        recs, stats, nrec = _gpu_frames(eng, torch, fmt, placed.torch_view(torch, at, cnt), first_frame_no=1 + at, new_file=(at == 0))
        assert gc.guards_intact(recs, nrec) and gc.guards_intact(stats, cnt)
        got.append(recs[:nrec]); gst.append(stats[:cnt])
        at += cnt
    eng.close()
    got, gst = np.concatenate(got), np.concatenate(gst)
    assert got.tobytes() == want.tobytes(), gc.first_difference(got, want)
    assert gst.tobytes() == wstats.tobytes(), gc.first_difference(gst, wstats)


@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(len(gc.LINE_SHAPES)), ids=LINE_IDS)
@pytest.mark.parametrize("fmt_name", FMT_NAMES)
def test_gpu_lines_in_awkward_buffers(fmt_name, idx, oracle_lib):
    placed, step, runs, mode = _placed_lines(fmt_name, idx)
    fmt = gc.FORMATS[fmt_name]
    eng, torch = _gpu_engine(mode)
    rows = placed.torch_view(torch)[0, ::step]
    assert rows.stride(0) == step * placed.row_stride and rows.stride(1) == 1
    k = fmt.recs_per_line
    for states, want, wscans in runs:
        out = _gpu_guarded(torch, len(want) + 2, fmt.rec_dtype.itemsize)
        d_st = torch.from_numpy(np.ascontiguousarray(states).view(np.uint8).reshape(len(states), 10)).to("cuda:0")
        scans = None
        if k == 1:
            eng.pcm1_binarize_lines(rows, d_st, frame_number=1, first_line=1, line_step=1, out_lines=out[:len(want)])
        else:
            _, scans = eng.pcm16x0_binarize_lines(rows, d_st, frame_number=1, first_line=1, line_step=1, out_lines=out[:len(want)], with_scan_done=True)
            scans = scans.cpu().numpy()
            assert len(scans) == len(wscans) and (scans == wscans).all()
        torch.cuda.synchronize()
        _check_lines(out.cpu().numpy().reshape(-1).view(fmt.rec_dtype), None, want, None)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pcm_type", FUSED, ids=FUSED_IDS)
def test_gpu_fused_call_in_an_awkward_buffer(pcm_type, oracle_lib):
    import stitch_api as sa
    from sdvpcmdecoder_amd import Pcm1StitchSettings, Pcm16x0StitchSettings
    from test_decode_frames import FRASM
    want = gc.fused_case(pcm_type)
    placed = gc.place(want[0], gc.FUSED_PAD, gc.FUSED_SHIFT, 0, seed=1090 + pcm_type)
    eng, torch = _gpu_engine(2)
    eng.setPCMType(pcm_type)
    eng.set_pcm1_stitch_settings(Pcm1StitchSettings.from_buffer_copy(bytes(gc.p1.default_settings())))
    eng.set_pcm16x0_stitch_settings(Pcm16x0StitchSettings.from_buffer_copy(bytes(gc.p16.default_settings())))
    n = gc.N_FRAMES
    cap, fcap, nst = (n + 2) * 1800 + 8192, n + 16, n + 1
    pairs, frames, stats = _gpu_guarded(torch, cap + 2, 12), _gpu_guarded(torch, fcap + 1, FRASM[pcm_type].itemsize), _gpu_guarded(torch, nst + 1, 32)
    view = placed.torch_view(torch)
    assert view.stride(1) == 720 + gc.FUSED_PAD and view.data_ptr() % 16 == gc.FUSED_SHIFT
    p, f, _s = eng.decode_frames(pcm_type, view, first_frame_no=1, new_file=True, end_file=True, out_pairs=pairs[:cap], out_frames=frames[:fcap], out_stats=stats[:nst])
    torch.cuda.synchronize()
    eng.close()
    _check_fused(pairs.cpu().numpy().reshape(-1).view(sa.PAIR_DTYPE), p.shape[0], frames.cpu().numpy().reshape(-1).view(FRASM[pcm_type]), f.shape[0],
                 stats.cpu().numpy(), nst, want)


@pytest.mark.gpu
def test_gpu_refuses_geometry_it_cannot_take():
    eng, torch = _gpu_engine(2)
    h, w, wide = 8, 720, gc.PX_BYTES + 1
    base = torch.zeros(2 * h * wide + 64, dtype=torch.uint8, device="cuda:0")
    for fmt in gc.FORMATS.values():
        frames_call = eng.pcm1_binarize_frames if fmt.name == "pcm1" else eng.pcm16x0_binarize_frames
        lines_call = eng.pcm1_binarize_lines if fmt.name == "pcm1" else eng.pcm16x0_binarize_lines
        for rs, fs, ww, n in ((w - 1, h * w, w, 1), (wide, h * wide, wide, 1), (w + 3, (h - 1) * (w + 3) + w - 1, w, 2)):
            nrec = int(getattr(eng.lib, fmt.count_fn)(h, n, 0))
            lines, stats = _gpu_guarded(torch, nrec + 2, fmt.rec_dtype.itemsize), _gpu_guarded(torch, n + 1, 32)
            with pytest.raises(RuntimeError, match=r"sdvpcm error -1:"):
                frames_call(torch.as_strided(base, (n, h, ww), (fs, rs, 1)), out_lines=lines[:nrec], out_stats=stats[:n])
            torch.cuda.synchronize()
            assert bool((lines == gc.GUARD).all()) and bool((stats == gc.GUARD).all()), (fmt.name, rs, fs, ww, n)
        for rs, ww in ((w - 1, w), (wide, wide)):
            out = _gpu_guarded(torch, 4 * fmt.recs_per_line + 2, fmt.rec_dtype.itemsize)
            with pytest.raises(RuntimeError, match=r"sdvpcm error -1:"):
                lines_call(torch.as_strided(base, (4, ww), (rs, 1)), None, out_lines=out[:4 * fmt.recs_per_line])
            torch.cuda.synchronize()
            assert bool((out == gc.GUARD).all()), (fmt.name, rs, ww)
    eng.close()
