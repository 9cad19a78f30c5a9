"""sdv_set_profiling (include/sdvpcm.h): the engine's own event timing of a call - sdv_run_info.kernel_ms of the frame entries, sdv_stitch_info.device_ms of
the stitch stage.  Switching it on changes nothing a call returns; the time it reports is above zero and below the wall clock of the call that measured
it; switched off the fields stay 0.  The STC-007 frame entry adds the time of every round (the damaged tape makes it run several), the other entries
set theirs once per call.  The fused entry does not queue its stitch stage ahead while profiling is on."""
import functools
import time

import numpy as np
import pytest

import dist_worker
from sdvpcmdecoder_amd.abi import PCM_PCM1 as PCM1, PCM_PCM16X0 as PCM16X0, PCM_STC007 as STC007

ENTRIES = ["binarize_frames", "pcm1_binarize_frames", "pcm16x0_binarize_frames", "stitch_frames", "decode_frames"]


@functools.lru_cache(maxsize=None)
def _tape(entry, damaged):
    """Four NTSC frames; damaged: one lost line in frame 1."""
    from sdvpcmdecoder_amd import synth
    if entry == "pcm1_binarize_frames":
        luma = dist_worker.pcm_tape("pcm1", 4)
    elif entry == "pcm16x0_binarize_frames":
        luma = dist_worker.pcm_tape("pcm16x0", 4)
    else:
        luma = synth.stc007_frames(4, seed=12, noise_sigma=4.0)[0]
    luma = np.ascontiguousarray(luma).copy()
    if damaged:
        luma[1, 77] = 16
    luma.setflags(write=False)
    return luma


def _timed(call):
    """(what the call returned, its wall clock in ms with the device idle before and after)"""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = call()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def _run(entry, luma, profiling):
    """-> (output bytes, reported times in ms, wall ms of the call that reported them, rounds of the frame stage, sdv_stitch_info.pipelined)"""
    import torch
    from sdvpcmdecoder_amd import Engine
    d = torch.from_numpy(luma.copy()).cuda()        # (the cached tape is read-only)
    eng = Engine(0)
    eng.set_profiling(profiling)
    kw = dict(first_frame_no=1, new_file=True, end_file=True)
    piped = 0
    if entry == "binarize_frames":
        eng.setPCMType(STC007)
        out, wall = _timed(lambda: eng.binarize_frames(d, **kw))
        times = [eng.run_info().kernel_ms]
    elif entry == "pcm1_binarize_frames":
        eng.setPCMType(PCM1)
        out, wall = _timed(lambda: eng.pcm1_binarize_frames(d, **kw))
        times = [eng.run_info().kernel_ms]
    elif entry == "pcm16x0_binarize_frames":
        eng.setPCMType(PCM16X0)
        out, wall = _timed(lambda: eng.pcm16x0_binarize_frames(d, **kw))
        times = [eng.run_info().kernel_ms]
    elif entry == "stitch_frames":
        eng.setPCMType(STC007)
        recs, _ = eng.binarize_frames(d, **kw)
        out, wall = _timed(lambda: eng.stitch_frames(recs))
        times = [eng.stitch_info().device_ms]
    else:
        eng.setPCMType(STC007)
        out, wall = _timed(lambda: eng.decode_frames(STC007, d, **kw))
        times = [eng.run_info().kernel_ms, eng.stitch_info().device_ms]
        piped = int(eng.stitch_info().pipelined)
    rounds = int(eng.run_info().rounds)
    return b"".join(t.cpu().numpy().tobytes() for t in out), [float(t) for t in times], wall, rounds, piped


@pytest.mark.gpu
@pytest.mark.parametrize("damaged", [False, True])
@pytest.mark.parametrize("entry", ENTRIES)
def test_gpu_profiling_reports_a_time_and_changes_nothing(entry, damaged):
    luma = _tape(entry, damaged)
    want, t_off, _, rounds_off, _ = _run(entry, luma, False)
    got, t_on, wall, rounds_on, piped = _run(entry, luma, True)
    print("%s %s: reported %s ms, wall %.3f ms, rounds %d; profiling off: %s" % (entry, "damaged" if damaged else "clean", t_on, wall, rounds_on, t_off))
    assert got == want and rounds_on == rounds_off
    assert all(t == 0.0 for t in t_off), t_off             # switched off: the fields stay as the call's start left them
    assert all(t > 0.0 for t in t_on), t_on
    assert sum(t_on) < wall, (t_on, wall)                   # the stages of a call run one after the other: their times lie inside its wall clock
    if damaged and entry in ("binarize_frames", "decode_frames"):
        assert rounds_on > 1, rounds_on                     # kernel_ms is the sum over the rounds
    assert piped & 4 == 0, piped


@pytest.mark.gpu
def test_gpu_profiling_switches_the_queueing_ahead_off():
    """A stream that plays, three frames per call: the fused entry queues the stitch stage of the later calls behind the frame kernel's first round
    (sdv_stitch_info.pipelined & 4) - not with profiling on, and the stream decodes to the same bytes either way."""
    import torch
    from sdvpcmdecoder_amd import Engine, synth
    d = torch.from_numpy(synth.stc007_frames(12, seed=12, noise_sigma=4.0)[0].copy()).cuda()
    outs, piped, times = {}, {}, []
    for profiling in (False, True):
        eng = Engine(0); eng.setPCMType(STC007)
        eng.set_profiling(profiling)
        outs[profiling], piped[profiling] = [], []
        for k in range(0, 12, 3):
            out, wall = _timed(lambda: eng.decode_frames(STC007, d[k:k + 3], first_frame_no=1 + k, new_file=k == 0, end_file=k + 3 == 12))
            outs[profiling].append(b"".join(t.cpu().numpy().tobytes() for t in out))
            piped[profiling].append(int(eng.stitch_info().pipelined))
            if profiling:
                times.append((float(eng.run_info().kernel_ms), float(eng.stitch_info().device_ms), wall))
    print("pipelined without / with profiling:", piped[False], piped[True], "times:", times)
    assert outs[True] == outs[False]
    assert any(x & 4 for x in piped[False]), piped
    assert not any(x & 4 for x in piped[True]), piped
    assert [x & 3 for x in piped[True]] == [x & 3 for x in piped[False]], piped       # otherwise the calls take the same way
    for k_ms, d_ms, wall in times:
        assert k_ms > 0.0 and d_ms > 0.0 and k_ms + d_ms < wall, times
