"""The builds of the STC-007 frame kernel and the shapes of sdv_binarize_lines that only the scheduler's history reaches, on the GPU against the sequential
oracle: the plain general build (worn tape) and its re-probe with the snapshots every eighth call, the worn-tape mark across calls, a round of more than 512
general frames whose sweeps are settled off the frame kernel, the emulator's scheduler tapes, and per-line calls past 65 536 lines and past the 16 384 lines of
a sweep chunk.  The developer build (libsdvpcm_hip_dev.so) counts the launches by build and proves that each tape reached the build it was made for."""
import ctypes as C
import functools
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_cases
import kernel_path_tapes as K
import libs
from oracle_run import oracle_binarize
from sdvpcmdecoder_amd import synth
from test_stc_lines import _oracle_lines, _states_behind
from pcm1_front_api import STATE_DTYPE
from sdvpcmdecoder_amd.abi import LF_REF_SWEEPED

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _tape(name):
    return K.TAPES[name]()


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """records, frame stats and the chain state the sequential oracle leaves after the whole stream"""
    luma, _ = _tape(name)
    recs, stats, state = oracle_binarize(luma, mode=2, return_state=True)
    return recs.tobytes(), stats.tobytes(), state.tobytes()


def _digest(recs, stats, state):
    return hashlib.sha256(bytes(recs) + bytes(stats) + bytes(state)).hexdigest()


def gpu_stream(luma, calls, counts=False):
    """One engine, the stream in calls of the given sizes: records, frame stats, chain state at the end, and per call (run info, launch counts or None)."""
    import torch
    import engine_api
    from sdvpcmdecoder_amd import Engine
    eng = Engine(0)
    eng.setBinarizationMode(2)
    d = torch.from_numpy(np.ascontiguousarray(luma)).to("cuda:0")

    def call(_chunk, first, new_file):
        lines, stats = eng.binarize_frames(d[first - 1:first - 1 + len(_chunk)], first_frame_no=first, new_file=new_file)
        torch.cuda.synchronize()
        extra = engine_api.launch_counts(eng.lib, eng._h) if counts else None
        return lines.cpu().numpy(), stats.cpu().numpy(), eng.run_info(), extra

    recs, stats, per_call = K.run_stream(call, luma, calls)
    state = eng.get_chain_state()
    eng.close()
    return recs.tobytes(), stats.tobytes(), state, per_call


@pytest.mark.parametrize("name", list(K.TAPES))
def test_gpu_tape_equals_the_sequential_oracle(name):
    """Records, frame descriptors and the chain state after the last call equal the oracle's over the whole stream; the run info of the calls says the
    scheduler took the way the tape was made for (the same checks as the emulator tests of these tapes)."""
    want = _oracle(name)            # (before the first GPU call)
    luma, calls = _tape(name)
    recs, stats, state, per_call = gpu_stream(luma, calls)
    assert recs == want[0], golden_cases.diff_report(np.frombuffer(recs, dtype=libs.LINE_DTYPE), np.frombuffer(want[0], dtype=libs.LINE_DTYPE))
    assert stats == want[1]
    assert state == want[2]
    info = [i for i, _ in per_call]
    if name in K.GPU_SCHEDULE:      # (what every call cost before the scheduler was split into a plan and a driver: the schedule itself, not only that it settles)
        assert [K.schedule_of(i) for i in info] == K.GPU_SCHEDULE[name]
    if name == "worn_plain_reprobe":
        assert all(i.frames_general >= 12 for i in info), [i.frames_general for i in info]
        assert [i.frames_met for i in info[1:8]] == [0] * 7 and info[9].frames_met == 0, [i.frames_met for i in info]      # (the plain build meets nothing)
    elif name == "worn_mark_comes_and_goes":
        assert info[1].frames_general == 0 and info[2].frames_general > 0, [i.frames_general for i in info]
        assert info[3].frames_general >= 12 and info[4].frames_general == 0, [i.frames_general for i in info]
    elif name == "big_round_with_sweeps":
        assert info[1].frames_general >= 600 and info[1].sweeps > 600, (info[1].frames_general, info[1].sweeps)
    elif name == "cold_chain_first_sweep":
        assert info[0].rounds == 2 and info[0].sweeps >= 1, (info[0].rounds, info[0].sweeps)
    elif name == "crowd_waits_for_first_frame":
        assert info[0].sweeps > 50, info[0].sweeps
    elif name == "general_kernel_later_shift_stage":
        assert info[0].frames_general >= 2
    elif name == "crowd_over_several_windows":
        assert info[1].rounds <= 8, info[1].rounds


@pytest.mark.parametrize("height,lpf", [(576, 294), (640, 320)])
def test_gpu_tall_frames_keep_their_histories(height, lpf):
    """test_emu_tall_frames_keep_their_histories on the GPU: more than 256 lines per field, a data window that moves half way; then a tape that plays is
    decoded in one round per call."""
    n = 8
    luma, _, _ = synth.stc007_frames(n_frames=n, seed=41, height=height, lines_per_field=lpf, noise_sigma=3.0)
    moved, _, _ = synth.stc007_frames(n_frames=n, seed=41, height=height, lines_per_field=lpf, noise_sigma=3.0, x0=17, x1=713)
    tape = np.concatenate([luma[:5], moved[5:], luma[:4]])
    want, want_stats, want_state = oracle_binarize(tape, mode=2, return_state=True)
    recs, stats, state, _ = gpu_stream(tape, [len(tape)])
    assert recs == want.tobytes(), golden_cases.diff_report(np.frombuffer(recs, dtype=libs.LINE_DTYPE), want)
    assert stats == want_stats.tobytes() and state == want_state.tobytes()
    steady, _, _ = synth.stc007_frames(n_frames=6, seed=42, height=height, lines_per_field=lpf, noise_sigma=3.0)
    stream = np.concatenate([steady, steady])
    want, want_stats = oracle_binarize(stream, mode=2)
    recs, stats, _, per_call = gpu_stream(stream, [6, 6])
    assert recs == want.tobytes() and stats == want_stats.tobytes()
    assert per_call[1][0].rounds == 1 and per_call[1][0].frames_general == 0


def test_gpu_bad_arguments():
    """test_emu_bad_arguments through the HIP library: the error codes and messages of sdv_binarize_frames, nothing launched."""
    import torch
    from sdvpcmdecoder_amd import Engine
    eng = Engine(0)
    lib, h = eng.lib, eng._h
    buf = torch.zeros((1, 8, 200), dtype=torch.uint8, device="cuda:0")
    recs = torch.zeros((11, 48), dtype=torch.uint8, device="cuda:0")
    st = torch.zeros((1, 32), dtype=torch.uint8, device="cuda:0")
    p = lambda t: C.c_void_p(t.data_ptr())
    f = lambda *a: lib.sdv_binarize_frames(h, *a, None)
    assert f(None, 200, 1600, 200, 8, 1, 1, 0, p(recs), 11, p(st), 1) == 1                  # SDV_ERR_NULL_VIDEO
    assert f(p(buf), 200, 1600, 200, 8, 1, 1, 0, None, 11, p(st), 1) == 2                   # SDV_ERR_NULL_PCM
    assert f(p(buf), 100, 800, 100, 8, 1, 1, 0, p(recs), 11, p(st), 1) == 3                 # SHORT_LINE
    assert b"137" in lib.sdv_last_error(h)
    assert f(p(buf), 200, 1600, 200, 8, 0, 1, 0, p(recs), 11, p(st), 1) == -1               # BAD_ARG
    assert f(p(buf), 200, 1600, 200, 8, 1, 1, 1, p(recs), 11, p(st), 1) == -1
    assert b"12 line records" in lib.sdv_last_error(h)
    assert f(p(buf), 200, 1600, 200, 8, 1, 1, 0, p(recs), 11, p(st), 0) == -1
    buf2 = torch.zeros((2, 8, 200), dtype=torch.uint8, device="cuda:0")
    recs2 = torch.zeros((22, 48), dtype=torch.uint8, device="cuda:0"); st2 = torch.zeros((2, 32), dtype=torch.uint8, device="cuda:0")
    assert f(p(buf2), 200, 1000, 200, 8, 2, 1, 0, p(recs2), 22, p(st2), 2) == -1
    assert b"frame_stride" in lib.sdv_last_error(h)
    torch.cuda.synchronize()
    assert not recs.any() and not st.any()
    eng.close()


def _lines_at_scale():
    """72 900 lines of a tape that plays: every fourth one cold (nothing tuned: it goes through the reference-level sweep), the others preset as a worker that
    hands every line that read on to its Binarizer would have them (_states_behind of the first lines of the tape, over and over)."""
    luma, _, _ = synth.stc007_frames(150, seed=17, noise_sigma=4.0)
    rows = np.ascontiguousarray(K.unreadable_cells(luma, every=97).reshape(-1, 720))
    head = _states_behind(_oracle_lines(rows[:486], None, 2), 2)
    states = np.resize(head, len(rows))
    cold = np.zeros(1, dtype=STATE_DTYPE)[0]
    cold["start"], cold["stop"] = -32768, 32767
    states[::4] = cold
    return rows, np.ascontiguousarray(states)


def test_gpu_lines_past_65536_and_past_a_sweep_chunk(oracle_lib):
    """sdv_binarize_lines on 72 900 lines in one call: the grid-stride loop of sdv_k_stc007_lines beyond 65 536 lines, more than 16 384 sweeps (two chunks of
    the sweep kernels), lines past LINES_PER_MEMO_FRAME swept from "frame" i / 16384.  Then on the same engine a call of 96 lines (its line buffers and memo
    heads left from the larger call) and a strided view (row_stride > width)."""
    import torch
    from sdvpcmdecoder_amd import Engine
    rows, states = _lines_at_scale()
    want = _oracle_lines(rows, states, 2, first_line=1, line_step=1, frame=3)
    swept = (want["flags"] & LF_REF_SWEEPED) != 0
    assert int(swept.sum()) > 16384 and int(swept[16384:].sum()) > 1000 and int(swept[65536:].sum()) > 100, int(swept.sum())
    small = rows[:96]
    want_small = _oracle_lines(small, None, 2, first_line=5, line_step=2, frame=9)
    want_field = _oracle_lines(np.ascontiguousarray(rows[:972:2]), None, 2, first_line=1, line_step=2, frame=4)
    eng = Engine(0)
    eng.setBinarizationMode(2)
    d = torch.from_numpy(rows).cuda()
    ds = torch.from_numpy(states.view(np.uint8).reshape(len(states), 10)).cuda()
    got = eng.binarize_lines(d, ds, frame_number=3, first_line=1, line_step=1).cpu().numpy().view(libs.LINE_DTYPE).reshape(-1)
    assert got.tobytes() == want.tobytes(), golden_cases.diff_report(got, want)
    got = eng.binarize_lines(d[:96], None, frame_number=9, first_line=5, line_step=2).cpu().numpy().view(libs.LINE_DTYPE).reshape(-1)
    assert got.tobytes() == want_small.tobytes(), golden_cases.diff_report(got, want_small)
    dv = d[:972:2]                  # (every second row: the odd field of two frames)
    assert dv.stride(0) == 1440
    got = eng.binarize_lines(dv, None, frame_number=4, first_line=1, line_step=2).cpu().numpy().view(libs.LINE_DTYPE).reshape(-1)
    assert got.tobytes() == want_field.tobytes(), golden_cases.diff_report(got, want_field)
    eng.close()


_DEV_SCRIPT = r"""
import json, os, sys, hashlib
sys.path[:0] = [sys.argv[1], os.path.join(sys.argv[1], "tests")]
import kernel_path_tapes as K
import test_gpu_kernel_paths as T
for name in K.TAPES:
    luma, calls = K.TAPES[name]()
    recs, stats, state, per_call = T.gpu_stream(luma, calls, counts=True)
    counts = [c for _, c in per_call]
    msg = K.check_counts(name, counts)
    assert msg is None, (name, msg, counts)
    print("COUNTS " + json.dumps({"tape": name, "digest": T._digest(recs, stats, state), "calls": [{k: v for k, v in c.items() if v} for c in counts]}), flush=True)
    for switch in K.SWITCHES:
        os.environ[switch] = "1"
        r2, s2, st2, pc2 = T.gpu_stream(luma, calls, counts=True)
        del os.environ[switch]
        assert (r2, s2, st2) == (recs, stats, state), (name, switch)
        msg = K.check_counts(name, [c for _, c in pc2], switch)
        assert msg is None, (name, switch, msg)
print("PATHS_OK")
"""


def test_gpu_kernel_paths_on_a_developer_build():
    """The same tapes through the developer build of the same sources (-DSDV_DEV_AIDS changes host code only) in a process of its own: the launch counts of
    every call show the build each tape was made for (engine.inc DevCount; kernel_path_tapes.check_counts), and every tape decoded again under each
    off-switch of the scheduler gives the same bytes as the default way - whose records, stats and chain state are the oracle's."""
    dev = os.path.join(ROOT, "sdvpcmdecoder_amd", "libsdvpcm_hip_dev.so")
    assert os.path.exists(dev), "no developer build of the HIP library (sdvpcmdecoder_amd/build.py: build_hip_dev, run by build())"
    want = {name: _digest(*_oracle(name)) for name in K.TAPES}
    env = dict(os.environ); env["SDVPCM_LIB"] = dev
    r = subprocess.run([sys.executable, "-c", _DEV_SCRIPT, ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "PATHS_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-4000:]
    seen = {}
    for line in r.stdout.splitlines():
        if line.startswith("COUNTS "):
            rec = json.loads(line[7:])
            seen[rec["tape"]] = rec["digest"]
            print(line)
    assert seen == want
