"""One tape sharded over two to five ranks (gloo, CPU, emulator build of the kernels): the concatenated per-rank output equals the
sequential decode of the whole tape by the oracle, whether the ranks' state predictions hold or have to be repaired - also where a
repair follows a repair (three ranks and more), where a range is a single frame, and where a warm-up reaches back to the tape's start.
The `gpu` twins run the same protocol with the product build: every rank a fresh process, all of them on device 0."""
import functools
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

import libs
import stitch_api as sa
from oracle_run import oracle_binarize
from sdvpcmdecoder_amd import synth
from sdvpcmdecoder_amd.sharded import shard_bounds

HERE = os.path.dirname(os.path.abspath(__file__))


def test_shard_bounds_cover_the_tape():
    for n in (1, 7, 10000, 100003):
        for w in (1, 2, 3, 8):
            b = [shard_bounds(n, r, w) for r in range(w)]
            assert b[0][0] == 0 and b[-1][1] == n and all(b[i][1] == b[i + 1][0] for i in range(w - 1))


@pytest.mark.parametrize("n_frames,warmup,s_warm,expect_redo", [(6, 3, 2, False), (10, 3, 2, True), (6, 3, 0, False)])
def test_two_ranks_one_tape(tmp_path, emu_lib, oracle_lib, n_frames, warmup, s_warm, expect_redo):
    world = 2
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(29500 + os.getpid() % 2000), WORLD_SIZE=str(world))
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "dist_worker.py"), str(tmp_path), str(n_frames), str(warmup), str(s_warm)],
                              env=dict(env, RANK=str(r), LOCAL_RANK=str(r))) for r in range(world)]
    for p in procs:
        assert p.wait(timeout=900) == 0
    # the sequential truth: the whole file through the oracle's two workers
    luma, _, _ = synth.stc007_frames(n_frames, seed=41, noise_sigma=3.0)
    recs, _ = oracle_binarize(luma, mode=2, new_file=True, end_file=True)
    want_p, want_f = sa.run_cpu(libs.load_oracle(), "orc_", recs, sa.default_settings())
    parts = [np.load(os.path.join(tmp_path, f"rank{r}.npz")) for r in range(world)]
    pairs = np.concatenate([np.ascontiguousarray(z["pairs"]).view(sa.PAIR_DTYPE).reshape(-1) for z in parts])
    frames = np.concatenate([np.ascontiguousarray(z["frames"]).view(sa.FRASM_DTYPE).reshape(-1) for z in parts])
    assert len(pairs) == len(want_p) and pairs.tobytes() == want_p.tobytes()
    assert len(frames) == len(want_f) and frames.tobytes() == want_f.tobytes()
    # a warm-up shorter than the predecessor's history cannot reproduce its coordinate history: the repair has to run
    assert (parts[1]["redo"][0] >= 1) == expect_redo, parts[1]["redo"]
    if s_warm == 0:         # a stitcher that starts cold cannot have guessed its predecessor's state: the range runs again from the true one
        assert parts[1]["redo"][1] >= 1, parts[1]["redo"]


def test_two_ranks_binarize_loop(tmp_path, emu_lib, oracle_lib):
    """What bench.py --gpus N times: batches of one continuing tape, each split over the ranks.  The geometry of the video changes
    from batch to batch, so ranks that simply carry on from their own previous state guess wrong and have to repair."""
    import ctypes as C
    n_frames, world = 4, 2
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(31500 + os.getpid() % 2000), WORLD_SIZE=str(world))
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "dist_worker.py"), str(tmp_path), str(n_frames), "-1", "0"],
                              env=dict(env, RANK=str(r), LOCAL_RANK=str(r))) for r in range(world)]
    for p in procs:
        assert p.wait(timeout=900) == 0
    lib = libs.load_oracle()
    lib.orc_v2d_new.restype = C.c_void_p
    h = C.c_void_p(lib.orc_v2d_new())
    lib.orc_v2d_set_mode.argtypes = [C.c_void_p, C.c_int]
    lib.orc_v2d_set_mode(h, 2)
    parts = [np.load(os.path.join(tmp_path, f"loop{r}.npz")) for r in range(world)]
    for batch in range(3):
        luma, _, _ = synth.stc007_frames(n_frames, seed=50 + batch, height=60, noise_sigma=3.0, x0=12 + 9 * batch, x1=700 - 5 * batch)
        want, _ = oracle_binarize(luma, handle=h, new_file=(batch == 0), first_frame_no=1 + batch * n_frames)
        got = np.concatenate([np.ascontiguousarray(z[f"b{batch}"]).view(libs.LINE_DTYPE).reshape(-1) for z in parts])
        assert got.tobytes() == want.tobytes(), f"batch {batch}"
    assert int(parts[1]["redo"]) >= 1


@pytest.mark.parametrize("fmt,n_frames,warmup,s_warm", [("pcm1", 6, 2, 2), ("pcm16x0", 6, 2, 2), ("pcm16x0_ei", 5, 1, 1), ("pcm1", 4, 0, 0), ("pcm16x0", 4, 0, 0)])
def test_two_ranks_one_pcm_tape(tmp_path, emu_lib, oracle_lib, fmt, n_frames, warmup, s_warm):
    """ShardedPcmDecoder: a PCM-1 / PCM-16x0 tape over two ranks equals the sequential decode by the oracle's two workers."""
    import dist_worker
    import pcm1_api as p1
    import pcm16_api as p16
    import pcm1_frames_api as p1f
    import pcm16_frames_api as p16f
    from test_pcm1 import bin_to_line_recs
    world = 2
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(33500 + os.getpid() % 2000), WORLD_SIZE=str(world))
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "dist_worker.py"), str(tmp_path), str(n_frames), str(warmup), str(s_warm), fmt],
                              env=dict(env, RANK=str(r), LOCAL_RANK=str(r))) for r in range(world)]
    for p in procs:
        assert p.wait(timeout=900) == 0
    luma = dist_worker.pcm_tape(fmt, n_frames)
    orc = libs.load_oracle()
    if fmt == "pcm1":
        recs, _ = p1f.run_cpu(orc, "orc_", luma, 2, dict(new_file=True, end_file=True))
        want_p, want_f = p1.run_cpu(orc, "orc_", bin_to_line_recs(recs), p1.default_settings())
        fdt = p1.FRASM1_DTYPE
    else:
        recs, _ = p16f.run_cpu(orc, "orc_", luma, 2, dict(new_file=True, end_file=True))
        want_p, want_f = p16.run_cpu(orc, "orc_", recs, p16.default_settings(format=1 if fmt == "pcm16x0_ei" else 0))
        fdt = p16.FRASM16_DTYPE
    parts = [np.load(os.path.join(tmp_path, f"rank{r}.npz")) for r in range(world)]
    pairs = np.concatenate([np.ascontiguousarray(z["pairs"]).view(sa.PAIR_DTYPE).reshape(-1) for z in parts])
    frames = np.concatenate([np.ascontiguousarray(z["frames"]).view(fdt).reshape(-1) for z in parts])
    assert len(pairs) == len(want_p) and pairs.tobytes() == want_p.tobytes()
    assert len(frames) == len(want_f) and frames.tobytes() == want_f.tobytes()
    assert all(int(z["redo"][2]) >= 1 for z in parts)
    if warmup == 0:         # no warm-up, no prediction: the second rank has to take its predecessor's real state and decode again
        assert int(parts[1]["redo"][0]) >= 1 and (fmt == "pcm1" or int(parts[1]["redo"][1]) >= 1), parts[1]["redo"]


# ---- the same loop in C++ (examples/decode_tape_sharded.cpp) ---------------------------------------------------------------------------------
def _sequential_truth(luma):
    recs, _ = oracle_binarize(luma, mode=2, new_file=True, end_file=True)
    return sa.run_cpu(libs.load_oracle(), "orc_", recs, sa.default_settings())


@pytest.mark.parametrize("n_frames,warmup,s_warm,expect_redo", [(6, 3, 2, False), (10, 3, 2, True)])
def test_cpp_host_program_two_ranks_one_tape(tmp_path, emu_lib, oracle_lib, n_frames, warmup, s_warm, expect_redo):
    """The C++ host program of the sharded decode, built against the emulator build of the engine, two processes, the all-gather through
    files: warm-up, all-gather of the 120-byte / 3.8 KB states through sdv_get_/set_*_state, verification and repair - the concatenated
    output is the oracle's sequential decode of the whole file, and the same as the Python harness gives (test_two_ranks_one_tape)."""
    from sdvpcmdecoder_amd import build as b
    exe = b.build_example_sharded_emu()
    luma, _, _ = synth.stc007_frames(n_frames, seed=41, noise_sigma=3.0)
    n, h, w = luma.shape
    (tmp_path / "luma.raw").write_bytes(np.ascontiguousarray(luma).tobytes())
    os.makedirs(tmp_path / "comm")
    world = 2
    procs = [subprocess.Popen([exe, str(tmp_path / "luma.raw"), str(w), str(h), str(n), str(tmp_path / "out"), "file:" + str(tmp_path / "comm"), str(warmup), str(s_warm)],
                              env=dict(os.environ, RANK=str(r), WORLD_SIZE=str(world)), stdout=subprocess.PIPE, text=True) for r in range(world)]
    outs = [p.communicate(timeout=900)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    want_p, want_f = _sequential_truth(luma)
    pairs = b"".join((tmp_path / f"out.rank{r}.pairs").read_bytes() for r in range(world))
    frames = b"".join((tmp_path / f"out.rank{r}.frames").read_bytes() for r in range(world))
    assert pairs == want_p.tobytes() and frames == want_f.tobytes()
    # a warm-up shorter than the predecessor's history cannot reproduce its coordinate history: the repair of the binarize stage has to run
    assert ("binarize 0," not in outs[1]) == expect_redo, outs[1]


@pytest.mark.gpu
def test_cpp_host_program_sharded_rccl_one_rank(tmp_path):
    """The product build on the GPU with one rank: ncclCommInitRank / ncclAllGather of the state blobs (the RCCL plumbing; more ranks need
    the multi-GPU node), output equal to the reference's for the file (tests/golden/e2e_ntsc_file.npz)."""
    from sdvpcmdecoder_amd import build as b
    import test_stitch_kernel as tsk
    exe = b.build_example_sharded()
    luma, z, want_p, want_f = tsk._e2e_fixture()
    n, h, w = luma.shape
    (tmp_path / "luma.raw").write_bytes(np.ascontiguousarray(luma).tobytes())
    out = subprocess.run([exe, str(tmp_path / "luma.raw"), str(w), str(h), str(n), str(tmp_path / "out"), "rccl"],
                         env=dict(os.environ, RANK="0", WORLD_SIZE="1", HSA_ENABLE_IPC_MODE_LEGACY="0"), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr + out.stdout
    assert "1 all-gathers" in out.stdout or "2 all-gathers" in out.stdout
    assert (tmp_path / "out.rank0.pairs").read_bytes() == want_p.tobytes()
    assert (tmp_path / "out.rank0.frames").read_bytes() == want_f.tobytes()


@pytest.mark.gpu
def test_cpp_host_program_sharded_two_ranks_one_gpu(tmp_path):
    """Two ranks of the product build sharing the one GPU of the test box, the all-gather through files (RCCL wants a GPU per rank): the
    device-side loop with real hand-over between the ranks."""
    from sdvpcmdecoder_amd import build as b
    import test_stitch_kernel as tsk
    exe = b.build_example_sharded()
    luma, z, want_p, want_f = tsk._e2e_fixture()
    n, h, w = luma.shape
    (tmp_path / "luma.raw").write_bytes(np.ascontiguousarray(luma).tobytes())
    os.makedirs(tmp_path / "comm")
    procs = [subprocess.Popen([exe, str(tmp_path / "luma.raw"), str(w), str(h), str(n), str(tmp_path / "out"), "file:" + str(tmp_path / "comm")],
                              env=dict(os.environ, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK="0"), stdout=subprocess.PIPE, text=True) for r in range(2)]
    outs = [p.communicate(timeout=600)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    assert b"".join((tmp_path / f"out.rank{r}.pairs").read_bytes() for r in range(2)) == want_p.tobytes()
    assert b"".join((tmp_path / f"out.rank{r}.frames").read_bytes() for r in range(2)) == want_f.tobytes()


@pytest.mark.gpu
def test_cpp_host_program_sharded_noisy_tape_decodes_no_range_twice(tmp_path):
    """A tape that plays with noise on it: the binarizer's levels are what the first lines of the tape measured (sticky), not what a warm-up further
    down would measure.  Rank 0 publishes its state after its first frames, rank 1 warms up from it: no range is decoded twice, and the two parts
    are the sequential decode."""
    from sdvpcmdecoder_amd import build as b
    exe = b.build_example_sharded()
    n = 150                 # (75 frames per rank: the stitcher's statistics rings, 65 deep, are full where rank 1 takes over, as its warm-up assumes)
    luma, _, _ = synth.stc007_frames(n, seed=77, noise_sigma=5.0)
    recs, _ = oracle_binarize(luma, mode=2, new_file=True, end_file=True)
    want_p, want_f = sa.run_cpu(libs.load_oracle(), "orc_", recs, sa.default_settings())
    _, h, w = luma.shape
    (tmp_path / "luma.raw").write_bytes(np.ascontiguousarray(luma).tobytes())
    os.makedirs(tmp_path / "comm")
    procs = [subprocess.Popen([exe, str(tmp_path / "luma.raw"), str(w), str(h), str(n), str(tmp_path / "out"), "file:" + str(tmp_path / "comm")],
                              env=dict(os.environ, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK="0"), stdout=subprocess.PIPE, text=True) for r in range(2)]
    outs = [p.communicate(timeout=600)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), outs
    assert all("ranges decoded again: binarize 0, stitch 0" in o for o in outs), outs
    assert b"".join((tmp_path / f"out.rank{r}.pairs").read_bytes() for r in range(2)) == want_p.tobytes()
    assert b"".join((tmp_path / f"out.rank{r}.frames").read_bytes() for r in range(2)) == want_f.tobytes()


@pytest.mark.gpu
def test_cpp_host_program_sharded_rccl_two_ranks(tmp_path):
    """Two ranks, a GPU each, ncclAllGather over the node's links (the multi-GPU node only: skipped on the one-GPU test boxes).  Run twice with the
    same output prefix and different run ids: the id file of the first run must not be picked up by the second (the rendezvous is per run)."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    from sdvpcmdecoder_amd import build as b
    import test_stitch_kernel as tsk
    exe = b.build_example_sharded()
    luma, z, want_p, want_f = tsk._e2e_fixture()
    n, h, w = luma.shape
    (tmp_path / "luma.raw").write_bytes(np.ascontiguousarray(luma).tobytes())
    for run in ("first", "second"):
        procs = [subprocess.Popen([exe, str(tmp_path / "luma.raw"), str(w), str(h), str(n), str(tmp_path / "out"), "rccl", "1", "1"],
                                  env=dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2", SDV_RUN_ID=run, HSA_ENABLE_IPC_MODE_LEGACY="0"),
                                  stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(2)]
        outs = [p.communicate(timeout=600) for p in procs]
        assert all(p.returncode == 0 for p in procs), outs
        assert not (tmp_path / "out.ncclid").exists()           # removed once both ranks had joined
        pairs = b"".join((tmp_path / f"out.rank{r}.pairs").read_bytes() for r in range(2))
        frames = b"".join((tmp_path / f"out.rank{r}.frames").read_bytes() for r in range(2))
        assert pairs == want_p.tobytes() and frames == want_f.tobytes()


# ---- three ranks and more ----------------------------------------------------------------------------------------------------------------------
# With two ranks nobody is successor and predecessor at once.  From three on a rank verifies its guess against a predecessor that is itself about
# to decode again (its final state changes under the successor: a repair that follows a repair), and a stitch repair is held back while a binarizer
# further up still decodes again.  The cases below reach those paths, ranges of one frame, ranges shorter than the warm-up and warm-ups that
# begin with the tape.
CPU_LIMIT = 300         # seconds for all ranks of a CPU run together (they take 5 .. 15 s; the limit only ends a deadlock)
PORT_STC, PORT_PCM, PORT_LOOP, PORT_EMPTY, PORT_GPU = 36000, 38000, 40000, 42000, 44000      # (+ pid % 2000: clear of 29500 / 31500 / 33500 above)


def _run_ranks(tmp_path, cmds, envs, limit, stop_on_failure=True):
    """Every rank a fresh child process, one time limit for the run.  A rank that exits non-zero (stop_on_failure) or the limit running out ends the
    run at once: whatever is still there is killed, nothing else is started.  -> exit codes (None: killed here), the ranks' output, timed out."""
    logs = [open(os.path.join(tmp_path, f"rank{r}.log"), "w+") for r in range(len(cmds))]
    procs, timed_out = [], False
    try:
        for cmd, env, log in zip(cmds, envs, logs):
            procs.append(subprocess.Popen(cmd, env=env, stdout=log, stderr=subprocess.STDOUT, text=True))
        deadline = time.monotonic() + limit
        while any(p.poll() is None for p in procs):
            if stop_on_failure and any(p.returncode not in (None, 0) for p in procs):
                break
            if time.monotonic() > deadline:
                timed_out = True
                break
            time.sleep(0.02)
        codes = [p.poll() for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        for p in procs:
            p.wait()
    outs = []
    for log in logs:
        log.seek(0)
        outs.append(log.read())
        log.close()
    return codes, outs, timed_out


def _run_workers(tmp_path, world, port, args, limit=CPU_LIMIT, **kw):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port + os.getpid() % 2000), WORLD_SIZE=str(world))
    cmd = [sys.executable, os.path.join(HERE, "dist_worker.py"), str(tmp_path)] + [str(a) for a in args]
    return _run_ranks(tmp_path, [cmd] * world, [dict(env, RANK=str(r), LOCAL_RANK=str(r)) for r in range(world)], limit, **kw)


def _ok(codes, outs, timed_out):
    assert not timed_out and all(c == 0 for c in codes), (codes, timed_out, [o[-2000:] for o in outs])


@functools.lru_cache(maxsize=None)
def _stc_truth(n_frames):
    """The sequential decode of the synth tape of dist_worker.py by the oracle's two workers (one run per tape length, shared by the cases)."""
    luma, _, _ = synth.stc007_frames(n_frames, seed=41, noise_sigma=3.0)
    want_p, want_f = _sequential_truth(luma)
    return want_p.tobytes(), want_f.tobytes()


def _check_parts(tmp_path, world, want_p, want_f):
    """-> the ranks' (binarize_redo, stitch_redo, gathers) rows, after the concatenated output was compared with the truth."""
    parts = [np.load(os.path.join(tmp_path, f"rank{r}.npz")) for r in range(world)]
    assert all(len(z["pairs"]) > 0 and len(z["frames"]) > 0 for z in parts), "a rank put out nothing"
    assert b"".join(np.ascontiguousarray(z["pairs"]).tobytes() for z in parts) == want_p
    assert b"".join(np.ascontiguousarray(z["frames"]).tobytes() for z in parts) == want_f
    redo = np.array([z["redo"] for z in parts])
    print("binarize_redo", redo[:, 0].tolist(), "stitch_redo", redo[:, 1].tolist(), "gathers", redo[:, 2].tolist())
    # every rank leaves the verify loop in the same round: one that left early would have deadlocked the others in the next all-gather
    assert len(set(redo[:, 2].tolist())) == 1 and redo[0, 2] >= 2, redo
    return redo


def _check_stc_redo(redo, warmup, s_warm, holds, cascade):
    bredo, sredo = redo[:, 0], redo[:, 1]
    assert bredo[0] == 0 and sredo[0] == 0, redo
    if holds:               # as the two-rank (6, 3, 2) case: no binarizer decodes twice
        assert (bredo == 0).all(), redo
    if s_warm == 0:         # a stitcher that starts cold cannot have guessed its predecessor's state (the two-rank case asserts it of rank 1)
        assert (sredo[1:] >= 1).all(), redo
    if cascade == "stitch":
        assert sredo[2:].max() >= 2, redo       # a repair behind a repair: the predecessor's final state changed under this rank
    if cascade == "binarize":
        assert bredo[2:].max() >= 2, redo


# world, frames, warm-up, stitcher warm-up, the binarizer predictions hold, the stage that cascades
STC_CASES = [
    pytest.param(3, 9, 3, 2, True, None, id="w3-predictions-hold"),
    # (rank 3 starts its warm-up, frames 3 .. 8, from rank 0's state behind frames 0 .. 2: a real prediction, f0 > 0, from the tape's first nine frames)
    pytest.param(4, 12, 6, 2, True, None, id="w4-predictions-hold"),
    pytest.param(4, 12, 3, 0, False, "stitch", id="w4-cold-stitcher-cascade"),
    pytest.param(4, 10, 1, 1, False, "binarize", id="w4-warmup1-cascade"),
    pytest.param(3, 3, 1, 1, False, None, id="w3-one-frame-ranges"),
    pytest.param(3, 3, 1, 0, False, None, id="w3-one-frame-ranges-cold-stitcher"),
    pytest.param(5, 5, 2, 2, False, None, id="w5-one-frame-ranges"),                       # the last rank: one frame, END_FILE, a stitcher warm-up
    pytest.param(5, 5, 2, 0, False, None, id="w5-one-frame-ranges-cold-stitcher"),
    pytest.param(3, 7, 2, 2, False, None, id="w3-uneven-2-2-3"),
    pytest.param(3, 6, 5, 2, True, None, id="w3-warmup-reaches-frame-0"),                  # ranks 1 and 2: f0 == 0, nothing inherited from rank 0
]


@pytest.mark.parametrize("world,n_frames,warmup,s_warm,holds,cascade", STC_CASES)
def test_more_ranks_one_tape(tmp_path, emu_lib, oracle_lib, world, n_frames, warmup, s_warm, holds, cascade):
    """ShardedDecoder over three to five ranks == the oracle's sequential decode, and the case reaches what it is there for."""
    _ok(*_run_workers(tmp_path, world, PORT_STC, [n_frames, warmup, s_warm]))
    redo = _check_parts(tmp_path, world, *_stc_truth(n_frames))
    _check_stc_redo(redo, warmup, s_warm, holds, cascade)


@pytest.mark.parametrize("world,warmup,s_warm", [(2, 1, 1), (3, 2, 2)])
def test_one_frame_last_range_keeps_its_turn_in_the_first_pass(emu_lib, oracle_lib, world, warmup, s_warm):
    """The last rank of `world` frames over `world` ranks, in this process: its one frame is the tape's last, it goes to the stitcher with the
    warm-up and the filler frame that closes the file is its successor.  The all-gather here answers that every predecessor ended in exactly what
    its successor assumed, so what the rank returns is its FIRST pass (in the runs over real ranks above the stitcher's guess is repaired and the
    last pass starts from a handed-over state - another path).  The warm-up begins with the tape (f0 == 0): the binarizer's state is the true one,
    and the rank's two descriptors (its frame, the END_FILE turn) and its pairs are the tail of the sequential decode."""
    import ctypes as C
    from sdvpcmdecoder_amd import build as b
    from sdvpcmdecoder_amd.sharded import ShardedDecoder
    from emu_engine_adapter import EmuEngine
    n_frames, rank = world, world - 1
    luma, _, _ = synth.stc007_frames(n_frames, seed=41, noise_sigma=3.0)
    want_p, want_f = _stc_truth(n_frames)

    def agreeing(blob):
        if len(blob) == 120:                # rank 0's early state: not used by a warm-up that begins with the tape
            return [blob] * world
        ns = (len(blob) - 240) // 2
        same = blob[:120] * 2 + blob[240:240 + ns] * 2        # (assumed, ended in) of both stages: what this rank assumed
        return [same] * rank + [blob]
    eng = EmuEngine(C.CDLL(b.build_emu()))
    eng.set_stitch_settings(sa.default_settings())
    dec = ShardedDecoder(eng, rank, world, agreeing, height=luma.shape[1], warmup=warmup, stitch_warmup=s_warm)
    f0, f1 = dec.frames_needed(n_frames)
    assert f0 == 0 and f1 == n_frames
    pairs, frames = dec.decode(luma[f0:f1], n_frames)
    eng.close()
    assert dec.stats == {"binarize_redo": 0, "stitch_redo": 0, "gathers": 2}
    assert len(frames) == 2 and frames.tobytes() == want_f[-2 * sa.FRASM_DTYPE.itemsize:]
    assert len(pairs) > 1470 and pairs.tobytes() == want_p[-len(pairs) * sa.PAIR_DTYPE.itemsize:]


@functools.lru_cache(maxsize=None)
def _pcm_truth(fmt, n_frames):
    import dist_worker
    import pcm1_api as p1
    import pcm16_api as p16
    import pcm1_frames_api as p1f
    import pcm16_frames_api as p16f
    from test_pcm1 import bin_to_line_recs
    luma = dist_worker.pcm_tape(fmt, n_frames)
    orc = libs.load_oracle()
    if fmt == "pcm1":
        recs, _ = p1f.run_cpu(orc, "orc_", luma, 2, dict(new_file=True, end_file=True))
        want_p, want_f = p1.run_cpu(orc, "orc_", bin_to_line_recs(recs), p1.default_settings())
    else:
        recs, _ = p16f.run_cpu(orc, "orc_", luma, 2, dict(new_file=True, end_file=True))
        want_p, want_f = p16.run_cpu(orc, "orc_", recs, p16.default_settings(format=1 if fmt == "pcm16x0_ei" else 0))
    return want_p.tobytes(), want_f.tobytes()


def _check_pcm_redo(redo, fmt, warmup):
    assert redo[0, 0] == 0 and redo[0, 1] == 0, redo
    if warmup == 0:         # no warm-up, no prediction: every rank behind the first takes its predecessor's real state and decodes again
        assert (redo[1:, 0] >= 1).all() and (fmt == "pcm1" or (redo[1:, 1] >= 1).all()), redo
    if fmt == "pcm1":       # PCM-1's stitcher carries nothing from frame to frame: nothing to repair
        assert (redo[:, 1] == 0).all(), redo


PCM_CASES = [(fmt, world, n, wu, sw) for fmt in ("pcm1", "pcm16x0", "pcm16x0_ei") for world, n, wu, sw in ((3, 7, 2, 2), (4, 8, 0, 0))] + [("pcm16x0", 4, 4, 1, 1)]


@pytest.mark.parametrize("fmt,world,n_frames,warmup,s_warm", PCM_CASES)
def test_more_ranks_one_pcm_tape(tmp_path, emu_lib, oracle_lib, fmt, world, n_frames, warmup, s_warm):
    """ShardedPcmDecoder over three and four ranks (uneven ranges; no warm-up at all; ranges of one frame) == the oracle's sequential decode."""
    _ok(*_run_workers(tmp_path, world, PORT_PCM, [n_frames, warmup, s_warm, fmt]))
    redo = _check_parts(tmp_path, world, *_pcm_truth(fmt, n_frames))
    _check_pcm_redo(redo, fmt, warmup)


@pytest.mark.parametrize("world,n_frames", [(3, 6), (4, 8)])
def test_more_ranks_binarize_loop(tmp_path, emu_lib, oracle_lib, world, n_frames):
    """ShardedBinarizeLoop over three and four ranks: the geometry changes from batch to batch, every rank behind the first guesses wrong,
    and a rank further down repairs twice in one batch (its predecessor's final state changed when that one repaired)."""
    import ctypes as C
    _ok(*_run_workers(tmp_path, world, PORT_LOOP, [n_frames, -1, 0]))
    lib = libs.load_oracle()
    lib.orc_v2d_new.restype = C.c_void_p
    h = C.c_void_p(lib.orc_v2d_new())
    lib.orc_v2d_set_mode.argtypes = [C.c_void_p, C.c_int]
    lib.orc_v2d_set_mode(h, 2)
    parts = [np.load(os.path.join(tmp_path, f"loop{r}.npz")) for r in range(world)]
    for batch in range(3):
        luma, _, _ = synth.stc007_frames(n_frames, seed=50 + batch, height=60, noise_sigma=3.0, x0=12 + 9 * batch, x1=700 - 5 * batch)
        want, _ = oracle_binarize(luma, handle=h, new_file=(batch == 0), first_frame_no=1 + batch * n_frames)
        got = np.concatenate([np.ascontiguousarray(z[f"b{batch}"]).view(libs.LINE_DTYPE).reshape(-1) for z in parts])
        assert got.tobytes() == want.tobytes(), f"batch {batch}"
    redo, gathers = [int(z["redo"]) for z in parts], [int(z["gathers"]) for z in parts]
    print("redo", redo, "gathers", gathers)
    assert len(set(gathers)) == 1, gathers
    assert redo[0] == 0 and all(r >= 1 for r in redo[1:]) and max(redo[2:]) >= 2, redo


@pytest.mark.parametrize("fmt", ["stc007", "pcm16x0"])
def test_fewer_frames_than_ranks_is_refused_by_every_rank(tmp_path, emu_lib, fmt):
    """Two frames over three ranks: rank 1 would own nothing.  Every rank says so and goes, before the first collective - a rank that gave up
    alone would leave the others waiting for it in the all-gather (the time limit is what a hang would run into)."""
    codes, outs, timed_out = _run_workers(tmp_path, 3, PORT_EMPTY, [2, 1, 1, fmt], limit=120, stop_on_failure=False)
    assert not timed_out, (codes, [o[-1000:] for o in outs])
    for r in range(3):
        assert codes[r] not in (None, 0), (r, codes)
        assert re.search(r"ValueError: .*\b2 frame.*\b3 rank", outs[r]), outs[r][-1000:]


# ---- the C++ host program, three ranks and more --------------------------------------------------------------------------------------------------
def _run_cpp(tmp_path, exe, luma, world, limit, extra=(), env=None):
    """`world` processes of the host program over one tape, the all-gather through files.  -> pairs, frames (concatenated), per rank (all-gathers,
    binarize ranges decoded again, stitch ranges decoded again)."""
    n, h, w = luma.shape
    (tmp_path / "luma.raw").write_bytes(np.ascontiguousarray(luma).tobytes())
    os.makedirs(tmp_path / "comm", exist_ok=True)
    cmd = [exe, str(tmp_path / "luma.raw"), str(w), str(h), str(n), str(tmp_path / "out"), "file:" + str(tmp_path / "comm")] + [str(a) for a in extra]
    envs = [dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), **(env or {})) for r in range(world)]
    _ok(*(res := _run_ranks(tmp_path, [cmd] * world, envs, limit)))
    stats = []
    for o in res[1]:
        m = re.search(r"(\d+) all-gathers, ranges decoded again: binarize (\d+), stitch (\d+)", o)
        assert m, o
        stats.append([int(m.group(2)), int(m.group(3)), int(m.group(1))])
    pairs = b"".join((tmp_path / f"out.rank{r}.pairs").read_bytes() for r in range(world))
    frames = b"".join((tmp_path / f"out.rank{r}.frames").read_bytes() for r in range(world))
    assert all((tmp_path / f"out.rank{r}.pairs").stat().st_size > 0 for r in range(world)), "a rank put out nothing"
    redo = np.array(stats)
    print("binarize_redo", redo[:, 0].tolist(), "stitch_redo", redo[:, 1].tolist(), "gathers", redo[:, 2].tolist())
    assert len(set(redo[:, 2].tolist())) == 1 and redo[0, 2] >= 2, redo
    return pairs, frames, redo


CPP_CASES = [STC_CASES[i] for i in (0, 2, 3, 4, 6)]


@pytest.mark.parametrize("world,n_frames,warmup,s_warm,holds,cascade", CPP_CASES)
def test_cpp_host_program_more_ranks_one_tape(tmp_path, emu_lib, oracle_lib, world, n_frames, warmup, s_warm, holds, cascade):
    """The C++ host program on the emulator build over three to five ranks: the same cases, the same output and the same verdicts as the Python
    harness - with the range that is the tape's last frame alone, behind a stitcher warm-up (five frames over five ranks)."""
    from sdvpcmdecoder_amd import build as b
    exe = b.build_example_sharded_emu()
    luma, _, _ = synth.stc007_frames(n_frames, seed=41, noise_sigma=3.0)
    pairs, frames, redo = _run_cpp(tmp_path, exe, luma, world, CPU_LIMIT, extra=(warmup, s_warm))
    want_p, want_f = _stc_truth(n_frames)
    assert pairs == want_p and frames == want_f
    _check_stc_redo(redo, warmup, s_warm, holds, cascade)


def test_cpp_host_program_four_ranks_reference_file(tmp_path, emu_lib):
    """The four frames of the reference's file over four ranks, default warm-ups (20 / 4): ranges of one frame, the last one the tape's last frame
    behind a stitcher warm-up.  The expected output is the real reference's (tests/golden/e2e_ntsc_file.npz)."""
    from sdvpcmdecoder_amd import build as b
    import test_stitch_kernel as tsk
    luma, z, want_p, want_f = tsk._e2e_fixture()
    pairs, frames, redo = _run_cpp(tmp_path, b.build_example_sharded_emu(), luma, 4, CPU_LIMIT)
    assert pairs == want_p.tobytes() and frames == want_f.tobytes()


def test_cpp_host_program_and_python_harness_reach_the_same_verdicts(tmp_path, emu_lib, oracle_lib):
    """The same tape, the same engine, the same protocol: every comparison of a guessed state with a handed-over one comes out the same in the C++
    program and in the Python harness, so both decode the same ranges again, in as many rounds.  (They did not while sdv_get_stitch_state exported
    the padding bytes of the hand-over chain as it found them: what lay there depended on the process, equal states compared unequal and rank 2 of
    the Python run repaired once more than its C++ twin.)"""
    from sdvpcmdecoder_amd import build as b
    world, n_frames, warmup, s_warm = 3, 9, 3, 2
    os.makedirs(tmp_path / "py")
    os.makedirs(tmp_path / "cpp")
    _ok(*_run_workers(tmp_path / "py", world, PORT_STC, [n_frames, warmup, s_warm]))
    want_p, want_f = _stc_truth(n_frames)
    py_redo = _check_parts(tmp_path / "py", world, want_p, want_f)
    luma, _, _ = synth.stc007_frames(n_frames, seed=41, noise_sigma=3.0)
    pairs, frames, cpp_redo = _run_cpp(tmp_path / "cpp", b.build_example_sharded_emu(), luma, world, CPU_LIMIT, extra=(warmup, s_warm))
    assert pairs == want_p and frames == want_f
    assert py_redo.tolist() == cpp_redo.tolist()


def test_cpp_host_program_fewer_frames_than_ranks_is_refused_by_every_rank(tmp_path, emu_lib):
    from sdvpcmdecoder_amd import build as b
    exe = b.build_example_sharded_emu()
    luma, _, _ = synth.stc007_frames(2, seed=41, height=60)
    n, h, w = luma.shape
    (tmp_path / "luma.raw").write_bytes(np.ascontiguousarray(luma).tobytes())
    os.makedirs(tmp_path / "comm")
    cmd = [exe, str(tmp_path / "luma.raw"), str(w), str(h), str(n), str(tmp_path / "out"), "file:" + str(tmp_path / "comm"), "1", "1"]
    codes, outs, timed_out = _run_ranks(tmp_path, [cmd] * 3, [dict(os.environ, RANK=str(r), WORLD_SIZE="3") for r in range(3)], 120, stop_on_failure=False)
    assert not timed_out, (codes, outs)
    for r in range(3):
        assert codes[r] not in (None, 0), (r, codes)
        assert re.search(r"\b2 frame.*\b3 rank", outs[r]), outs[r]


# ---- GPU twins: the product build, every rank a fresh process, all on device 0 ---------------------------------------------------------------------
# The time limits: four times what test_cpp_host_program_sharded_two_ranks_one_gpu takes for the runs of four ranks, eight times for
# the runs of five and of eight - the ranks of a run share one GPU and 16 CPUs.  NOT MEASURED YET: no MI355X could be had when these tests were written, so
# GPU_TWO_RANKS_S is a quarter of the 600 s the two-rank tests above allow themselves, not a duration.  Put the measured figure here at the first
# run on the GPU box.  The parent never opens the GPU itself.
GPU_TWO_RANKS_S = 150.0
GPU_LIMIT_4, GPU_LIMIT_8 = 4 * GPU_TWO_RANKS_S, 8 * GPU_TWO_RANKS_S


def _gpu_example():
    from sdvpcmdecoder_amd import build as b
    return b.build_example_sharded()


@pytest.mark.gpu
def test_cpp_host_program_sharded_four_ranks_one_gpu(tmp_path):
    """The four frames of the reference's file over four ranks of the product build, default warm-ups: every range is one frame, the last rank's
    is the tape's last frame behind a stitcher warm-up.  The expected output is the real reference's (tests/golden/e2e_ntsc_file.npz)."""
    import test_stitch_kernel as tsk
    luma, z, want_p, want_f = tsk._e2e_fixture()
    pairs, frames, redo = _run_cpp(tmp_path, _gpu_example(), luma, 4, GPU_LIMIT_4, env=dict(LOCAL_RANK="0"))
    assert pairs == want_p.tobytes() and frames == want_f.tobytes()


@pytest.mark.gpu
def test_cpp_host_program_sharded_eight_ranks_one_gpu(tmp_path, oracle_lib):
    """Eight ranks of the product build on one GPU (the reference's file has four frames - fewer than ranks, which is refused -, so the tape is
    the 16-frame synth tape and the truth the oracle's): a cold stitcher on every rank, so repairs run down the whole chain of ranks."""
    pairs, frames, redo = _run_cpp(tmp_path, _gpu_example(), synth.stc007_frames(16, seed=41, noise_sigma=3.0)[0], 8, GPU_LIMIT_8, extra=(3, 0), env=dict(LOCAL_RANK="0"))
    want_p, want_f = _stc_truth(16)
    assert pairs == want_p and frames == want_f
    _check_stc_redo(redo, 3, 0, False, "stitch")


@pytest.mark.gpu
def test_cpp_host_program_sharded_one_frame_ranges_one_gpu(tmp_path, oracle_lib):
    """Five frames over five ranks of the product build, warm-ups of two: the twin of the CPU case w5-one-frame-ranges."""
    pairs, frames, redo = _run_cpp(tmp_path, _gpu_example(), synth.stc007_frames(5, seed=41, noise_sigma=3.0)[0], 5, GPU_LIMIT_8, extra=(2, 2), env=dict(LOCAL_RANK="0"))
    want_p, want_f = _stc_truth(5)
    assert pairs == want_p and frames == want_f


@pytest.mark.gpu
@pytest.mark.parametrize("n_frames,warmup,s_warm,holds,cascade", [(12, 6, 2, True, None), (12, 3, 0, False, "stitch")])
def test_four_ranks_one_tape_one_gpu(tmp_path, oracle_lib, n_frames, warmup, s_warm, holds, cascade):
    """ShardedDecoder with the product's Engine: four ranks on device 0, the all-gather over gloo - the twins of w4-predictions-hold and
    w4-cold-stitcher-cascade."""
    _ok(*_run_workers(tmp_path, 4, PORT_GPU, [n_frames, warmup, s_warm, "stc007", "hip"], limit=GPU_LIMIT_4))
    redo = _check_parts(tmp_path, 4, *_stc_truth(n_frames))
    _check_stc_redo(redo, warmup, s_warm, holds, cascade)


@pytest.mark.gpu
def test_four_ranks_one_pcm16x0_tape_one_gpu(tmp_path, oracle_lib):
    """ShardedPcmDecoder with the product's Engine: a PCM-16x0 tape, uneven ranges, four ranks on device 0."""
    _ok(*_run_workers(tmp_path, 4, PORT_GPU, [7, 2, 2, "pcm16x0", "hip"], limit=GPU_LIMIT_4))
    redo = _check_parts(tmp_path, 4, *_pcm_truth("pcm16x0", 7))
    _check_pcm_redo(redo, "pcm16x0", 2)
