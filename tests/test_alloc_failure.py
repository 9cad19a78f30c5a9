"""A call that fails at an allocation leaves its engine usable (csrc/engine.inc, rt::DevBuf / rt::PinBuf).

The emulator build can be told to fail its n-th next allocation once (sdv_emu_fail_alloc, tests/emu/emu_engine.cpp).  For every allocation a large
call makes on a fresh engine - counted in a clean run, not written down here - that call is made to fail there: it returns SDV_ERR_HIP, and a
smaller call on the same engine then succeeds with the bytes of the oracle and of a fresh engine.  A buffer whose capacity outlived its memory, or a
group of buffers grown by half, would hand the smaller call a NULL or a too small buffer."""
import ctypes as C

import numpy as np
import pytest

import engine_api as ea
import kernel_path_tapes as kt
import libs
import pcm1_api as p1
import pcm16_api as p16
import stitch_api as sa
import stitch_cases as sc
from oracle_run import oracle_binarize
from sdvpcmdecoder_amd.abi import ERR_HIP as SDV_ERR_HIP

FAR = 1 << 30


def _binarize_case(emu_lib):
    big, small = kt.worn_tape(10, 64), kt.worn_tape(3, 64, seed=32)       # damage in every frame: the sweep pool and the snapshots are in play
    want = oracle_binarize(small, mode=2)

    def call(eng, luma):
        emu_lib.sdv_set_mode(eng, 2)
        rc, recs, stats = ea.emu_binarize(emu_lib, eng, luma)
        return rc, (recs.tobytes(), stats.tobytes())

    def check_clean(eng):
        info = ea.RunInfo()
        assert emu_lib.sdv_get_run_info(eng, C.byref(info)) == 0
        assert info.sweeps > 0 and info.frames_general > 0, "the tape did not reach the sweep pool"
    return big, small, (want[0].tobytes(), want[1].tobytes()), call, lambda eng: emu_lib.sdv_reset_stream(eng), check_clean


def _stitch_case(emu_lib):
    big, st_big = sc.make_input("ntsc_drift", lambda luma: oracle_binarize(luma, mode=2))
    small, st_small = sc.make_input("ntsc_bad10_no_pq", lambda luma: oracle_binarize(luma, mode=2))
    want = sa.run_cpu(libs.load_oracle(), "orc_", small, st_small)

    def call(eng, recs):
        rc, pairs, frames = ea.emu_stitch(emu_lib, eng, recs, st_big if recs is big else st_small)
        return rc, (pairs.tobytes(), frames.tobytes())
    return big, small, (want[0].tobytes(), want[1].tobytes()), call, lambda eng: emu_lib.sdv_reset_stitcher(eng), None


def _pcm1_case(emu_lib):
    big, st_big = p1.make_input("manual_lost_many")         # manual line offsets: the field buffers that outlive a frame as well
    small, st_small = p1.make_input("clean")
    want = p1.run_cpu(libs.load_oracle(), "orc_", small, st_small)

    def call(eng, recs):
        rc, pairs, frames = ea.emu_pcm1_stitch(emu_lib, eng, recs, st_big if recs is big else st_small)
        return rc, (pairs.tobytes(), frames.tobytes())
    return big, small, (want[0].tobytes(), want[1].tobytes()), call, None, None


def _pcm16_case(emu_lib):
    big, st_big = p16.make_input("ei_wander")
    small, st_small = p16.make_input("si_bad10")
    want = p16.run_cpu(libs.load_oracle(), "orc_", small, st_small)

    def call(eng, recs):
        rc, pairs, frames = ea.emu_pcm16_stitch(emu_lib, eng, recs, st_big if recs is big else st_small)
        return rc, (pairs.tobytes(), frames.tobytes())
    return big, small, (want[0].tobytes(), want[1].tobytes()), call, None, None


@pytest.mark.parametrize("case", [_binarize_case, _stitch_case, _pcm1_case, _pcm16_case], ids=["binarize_frames", "stitch_frames", "pcm1_stitch_frames", "pcm16x0_stitch_frames"])
def test_failed_allocation_leaves_engine_usable(case, emu_lib, oracle_lib):
    big, small, want, call, reset, check_clean = case(emu_lib)
    # a fresh engine: what the small call gives, and how many allocations the large one makes
    eng = emu_lib.sdv_engine_create(0)
    rc, fresh = call(eng, small)
    emu_lib.sdv_engine_destroy(eng)
    assert rc == 0 and fresh == want, "the emulator differs from the oracle without any failure"
    eng = emu_lib.sdv_engine_create(0)
    emu_lib.sdv_emu_fail_alloc(FAR)
    rc, _ = call(eng, big)
    n_allocs = FAR - emu_lib.sdv_emu_fail_alloc(0)
    assert rc == 0, emu_lib.sdv_last_error(eng)
    if check_clean:
        check_clean(eng)
    emu_lib.sdv_engine_destroy(eng)
    assert n_allocs >= 4, "the large call allocates nothing?"
    for k in range(1, n_allocs + 1):
        eng = emu_lib.sdv_engine_create(0)
        emu_lib.sdv_emu_fail_alloc(k)
        rc, _ = call(eng, big)
        left = emu_lib.sdv_emu_fail_alloc(0)
        assert left == 0, f"allocation {k} of {n_allocs} was never asked for"
        assert rc == SDV_ERR_HIP, f"allocation {k} of {n_allocs} failed and the call returned {rc}"
        if reset:
            assert reset(eng) == 0          # (the stream starts again: what a failed call leaves of it is not under test here)
        rc, got = call(eng, small)
        assert rc == 0, f"after a failure at allocation {k} of {n_allocs}: {emu_lib.sdv_last_error(eng)}"
        assert got == want, f"after a failure at allocation {k} of {n_allocs} the smaller call differs from the oracle"
        emu_lib.sdv_engine_destroy(eng)
