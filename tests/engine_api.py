"""ctypes binding of the C-ABI in include/sdvpcm.h, usable with either the product library
(sdvpcmdecoder_amd/libsdvpcm_hip.so, device pointers) or the test-only emulator build
(tests/emu/libsdvpcm_emu.so, host pointers)."""
import ctypes as C
import numpy as np
import libs

from sdvpcmdecoder_amd import abi
from sdvpcmdecoder_amd.abi import STATS_DTYPE, RunInfo, StitchInfo  # noqa: F401

bind = abi.bind      # every prototype of include/sdvpcm.h, on whichever build `lib` is


def emu_stitch(lib, eng, recs, settings=None, pair_cap=None, frame_cap=None):
    """Host-memory call (emulator build only): one sdv_stitch_frames call over `recs`."""
    import stitch_api as sa
    if settings is not None:
        assert lib.sdv_set_stitch_settings(eng, C.byref(settings)) == 0
    recs = np.ascontiguousarray(recs)
    nfr = int((recs["service_type"] == 5).sum()) + 2
    pair_cap = pair_cap or nfr * 2400 + 16
    frame_cap = frame_cap or nfr * 3
    pairs = np.zeros(pair_cap, dtype=sa.PAIR_DTYPE)
    frames = np.zeros(frame_cap, dtype=sa.FRASM_DTYPE)
    npairs, nframes = C.c_size_t(0), C.c_size_t(0)
    rc = lib.sdv_stitch_frames(eng, recs.ctypes.data, len(recs), pairs.ctypes.data, pair_cap, C.byref(npairs),
                               frames.ctypes.data, frame_cap, C.byref(nframes), None)
    return rc, pairs[:npairs.value], frames[:nframes.value]


def emu_pcm1_stitch(lib, eng, recs, settings=None, pair_cap=None, frame_cap=None):
    """Host-memory call (emulator build only): one sdv_pcm1_stitch_frames call over `recs`."""
    import pcm1_api as p1
    import stitch_api as sa
    if settings is not None:
        assert lib.sdv_set_pcm1_stitch_settings(eng, C.byref(settings)) == 0
    recs = np.ascontiguousarray(recs)
    nfr = int((recs["service_type"] == 5).sum()) + 2
    pair_cap = pair_cap or nfr * 1472 + 16
    frame_cap = frame_cap or nfr + 8
    pairs = np.zeros(pair_cap, dtype=sa.PAIR_DTYPE)
    frames = np.zeros(frame_cap, dtype=p1.FRASM1_DTYPE)
    npairs, nframes = C.c_size_t(0), C.c_size_t(0)
    rc = lib.sdv_pcm1_stitch_frames(eng, recs.ctypes.data if len(recs) else None, len(recs), pairs.ctypes.data, pair_cap, C.byref(npairs),
                                    frames.ctypes.data, frame_cap, C.byref(nframes), None)
    return rc, pairs[:min(npairs.value, pair_cap)], frames[:min(nframes.value, frame_cap)]


def emu_pcm1_stitch_vis(lib, eng, recs, settings=None, blocks=True, lines=True, block_cap=None, line_cap=None):
    """... with the visualiser's feeds switched on (sdv_set_pcm1_stitch_block_output / _line_output): (rc, pairs, frames, blocks, sub-lines)."""
    import pcm1_api as p1
    nfr = int((recs["service_type"] == 5).sum()) + 2
    bl = np.zeros(block_cap if block_cap is not None else nfr * 16, dtype=p1.BLOCK1_DTYPE)
    ln = np.zeros(line_cap if line_cap is not None else nfr * 1470, dtype=p1.ASM1_DTYPE)
    assert lib.sdv_set_pcm1_stitch_block_output(eng, bl.ctypes.data if blocks else None, len(bl)) == 0
    assert lib.sdv_set_pcm1_stitch_line_output(eng, ln.ctypes.data if lines else None, len(ln)) == 0
    rc, pairs, frames = emu_pcm1_stitch(lib, eng, recs, settings)
    nb, nl = lib.sdv_pcm1_stitch_block_count(eng), lib.sdv_pcm1_stitch_line_count(eng)
    emu_pcm1_stitch_vis.last_counts = (nb, nl)          # what the call made (or needed)
    assert lib.sdv_set_pcm1_stitch_block_output(eng, None, 0) == 0 and lib.sdv_set_pcm1_stitch_line_output(eng, None, 0) == 0
    return rc, pairs, frames, bl[:min(nb, len(bl))].copy(), ln[:min(nl, len(ln))].copy()


def emu_pcm16_stitch_vis(lib, eng, recs, settings=None, block_cap=None):
    """... with the visualiser's block feed switched on (sdv_set_pcm16x0_stitch_block_output): (rc, pairs, frames, blocks)."""
    import pcm16_api as p16
    nfr = int((recs["service_type"] == 5).sum()) + 2
    bl = np.zeros(block_cap if block_cap is not None else nfr * 800 + 16, dtype=p16.VBLOCK16_DTYPE)
    assert lib.sdv_set_pcm16x0_stitch_block_output(eng, bl.ctypes.data, len(bl)) == 0
    rc, pairs, frames = emu_pcm16_stitch(lib, eng, recs, settings)
    nb = lib.sdv_pcm16x0_stitch_block_count(eng)
    emu_pcm16_stitch_vis.last_count = nb
    assert lib.sdv_set_pcm16x0_stitch_block_output(eng, None, 0) == 0
    return rc, pairs, frames, bl[:min(nb, len(bl))].copy()


def emu_pcm16_stitch_lines(lib, eng, recs, settings=None, line_cap=None):
    """... with the assembled sub-lines switched on (sdv_set_pcm16x0_stitch_line_output): (rc, pairs, frames, lines)."""
    nfr = int((recs["service_type"] == 5).sum()) + 2
    ln = np.zeros(line_cap if line_cap is not None else nfr * 3000 + 16, dtype=recs.dtype)
    assert lib.sdv_set_pcm16x0_stitch_line_output(eng, ln.ctypes.data, len(ln)) == 0
    rc, pairs, frames = emu_pcm16_stitch(lib, eng, recs, settings)
    nl = lib.sdv_pcm16x0_stitch_line_count(eng)
    emu_pcm16_stitch_lines.last_count = nl
    assert lib.sdv_set_pcm16x0_stitch_line_output(eng, None, 0) == 0
    return rc, pairs, frames, ln[:min(nl, len(ln))].copy()


def emu_pcm16_stitch(lib, eng, recs, settings=None, pair_cap=None, frame_cap=None):
    """Host-memory call (emulator build only): one sdv_pcm16x0_stitch_frames call over `recs`."""
    import pcm16_api as p16
    import stitch_api as sa
    if settings is not None:
        assert lib.sdv_set_pcm16x0_stitch_settings(eng, C.byref(settings)) == 0
    recs = np.ascontiguousarray(recs)
    nfr = int((recs["service_type"] == 5).sum()) + 2
    pair_cap = pair_cap or nfr * 1472 + 16
    frame_cap = frame_cap or nfr + 8
    pairs = np.zeros(pair_cap, dtype=sa.PAIR_DTYPE)
    frames = np.zeros(frame_cap, dtype=p16.FRASM16_DTYPE)
    npairs, nframes = C.c_size_t(0), C.c_size_t(0)
    rc = lib.sdv_pcm16x0_stitch_frames(eng, recs.ctypes.data if len(recs) else None, len(recs), pairs.ctypes.data, pair_cap, C.byref(npairs),
                                       frames.ctypes.data, frame_cap, C.byref(nframes), None)
    return rc, pairs[:min(npairs.value, pair_cap)], frames[:min(nframes.value, frame_cap)]


def emu_binarize(lib, eng, luma, first_frame_no=1, flags=1, row_stride=None, misalign=0):
    """Host-memory call (emulator build only).  row_stride / misalign: the same pixels in a padded, shifted buffer."""
    n, h, w = luma.shape
    if row_stride is not None or misalign:
        rs = row_stride or w
        buf = np.full(n * h * rs + misalign + 64, 0x5A, dtype=np.uint8)
        view = buf[misalign:misalign + n * h * rs].reshape(n, h, rs)
        view[:, :, :w] = luma
        nrec = n * (h + 3) + (1 if flags & 1 else 0) + (h + 4 if flags & 4 else 0)
        recs = np.zeros(nrec, dtype=libs.LINE_DTYPE)
        stats = np.zeros(n + (1 if flags & 4 else 0), dtype=STATS_DTYPE)
        rc = lib.sdv_binarize_frames(eng, buf.ctypes.data + misalign, rs, rs * h, w, h, n, first_frame_no, flags, recs.ctypes.data, len(recs),
                                     stats.ctypes.data, len(stats), None)
        return rc, recs, stats
    nrec = n * (h + 3) + (1 if flags & 1 else 0) + (h + 4 if flags & 4 else 0)
    recs = np.zeros(nrec, dtype=libs.LINE_DTYPE)
    stats = np.zeros(n + (1 if flags & 4 else 0), dtype=STATS_DTYPE)
    luma = np.ascontiguousarray(luma)
    rc = lib.sdv_binarize_frames(eng, luma.ctypes.data, w, w * h, w, h, n, first_frame_no, flags, recs.ctypes.data, len(recs),
                                 stats.ctypes.data, len(stats), None)
    return rc, recs, stats


LAUNCH_COUNT_NAMES = ("lean", "lean_frames", "snap", "snap_frames", "plain", "plain_frames", "fat", "fat_frames",
                      "sweep_levels", "sweep_levels_reqs", "sweep_pick", "sweep_pick_reqs", "lines", "lines_lines")


def launch_counts(lib, eng):
    """Developer builds only (SDV_DEV_AIDS: the emulator build, libsdvpcm_hip_dev.so): the launches of the last sdv_binarize_frames /
    sdv_binarize_lines call by kernel build, and the frames / sweep requests / lines they were given (sdv_dev_launch_counts, engine.inc DevCount)."""
    f = lib.sdv_dev_launch_counts
    out = (C.c_uint32 * len(LAUNCH_COUNT_NAMES))()
    assert f(eng, out, len(out)) == len(LAUNCH_COUNT_NAMES)
    return dict(zip(LAUNCH_COUNT_NAMES, (int(x) for x in out)))
