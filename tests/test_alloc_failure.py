"""A call that fails at an allocation leaves its engine usable (csrc/engine.inc, rt::DevBuf / rt::PinBuf).

The emulator build can be told to fail its n-th next allocation once (sdv_emu_fail_alloc, tests/emu/emu_engine.cpp).  For every allocation a large
call makes on a fresh engine - counted in a clean run, not written down here - that call is made to fail there: it returns SDV_ERR_HIP, and a
smaller call on the same engine then succeeds with the bytes of the oracle and of a fresh engine.  A buffer whose capacity outlived its memory, or a
group of buffers grown by half, would hand the smaller call a NULL or a too small buffer.

The sample-stream stages promise more (include/sdvpcm.h): a failed call leaves the stream where it was.  test_failed_allocation_keeps_the_stream makes
every allocation of every call of a stream fail once and repeats that call on the same engine, without a reset: the stream's bytes are the clean run's."""
import ctypes as C

import numpy as np
import pytest

import audio_api as A
import engine_api as ea
import kernel_path_tapes as kt
import libs
import pcm1_api as p1
import pcm16_api as p16
import stitch_api as sa
import stitch_cases as sc
from oracle_run import oracle_binarize
from sdvpcmdecoder_amd import abi
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


# ---- the sample-stream stages: the stream survives a failed call ----------------------------------------------------------------------------------
STREAM_CUTS = (0, 300, 9000)            # a stream of 9000 pairs in two calls; the second one ends it (stop / flush) where the call has such an argument


# the streams of the cases below, 9000 pairs each (tests/memory_history.py runs the same ones)
def audio_process_tape():
    # dropouts for the linear mode to work on, and an END_FILE / NEW_FILE pair in the second call: three stretches, and the purge drops a pair, so
    # the output does not lie where the work array has it (the staged path)
    return A.tape([A.audio(4000, 41, runs=((100, 3, 0), (2000, 5, 2)), p_bad=0.01), "E", "N", A.audio(4998, 42, runs=((4000, 4, 1),), p_bad=0.01)])


def deemphasis_tape():
    return A.audio(9000, 43, emphasis=1)


def resample_tape():
    return A.audio(9000, 44)


def pcm_tape():
    return np.random.default_rng(45).integers(-20000, 20001, (9000, 2)).astype(np.int16)


def _audio_process_stream(lib):
    pairs = audio_process_tape()

    def setup(eng):
        assert lib.sdv_set_audio_masking(eng, abi.DROP_INTER_LIN_WORD) == 0

    def call(eng, a, b, last):
        rc, out, pur, masked, _, _ = A.emu_audio(lib, eng, pairs[a:b], 1 if last else 0)
        return rc, out.tobytes() + pur.tobytes() + masked.to_bytes(8, "little")
    return setup, call


def _deemphasis_stream(lib):
    pairs = deemphasis_tape()

    def setup(eng):
        assert lib.sdv_set_deemphasis(eng, abi.DEEMPH_FORCE) == 0

    def call(eng, a, b, last):
        src, out = np.ascontiguousarray(pairs[a:b]), np.zeros(b - a, dtype=A.PAIR_DTYPE)
        return lib.sdv_audio_deemphasis(eng, src.ctypes.data, b - a, out.ctypes.data, None), out.tobytes()
    return setup, call


def _resample_stream(mode):
    def case(lib):
        pairs = resample_tape()

        def setup(eng):
            assert lib.sdv_set_resample(eng, mode) == 0

        def call(eng, a, b, last):
            cap = lib.sdv_audio_resample_room(eng, b - a)
            src, out, n_out = np.ascontiguousarray(pairs[a:b]), np.zeros(cap + 1, dtype=A.PAIR_DTYPE), C.c_size_t(0)
            rc = lib.sdv_audio_resample(eng, src.ctypes.data, b - a, 1 if last else 0, out.ctypes.data, cap, C.byref(n_out), None)
            return rc, out[:n_out.value].tobytes()
        return setup, call
    return case


def _pcm_stream(resample):
    def case(lib):
        pcm = pcm_tape()

        def call(eng, a, b, last):
            src = np.ascontiguousarray(pcm[a:b])
            if not resample:
                out = np.zeros((b - a, 2), dtype=np.int16)
                return lib.sdv_pcm_preemphasis(eng, src.ctypes.data, b - a, 44100, out.ctypes.data, None), out.tobytes()
            cap = lib.sdv_pcm_resample_room(eng, b - a)
            out, n_out = np.zeros((cap + 1, 2), dtype=np.int16), C.c_size_t(0)
            rc = lib.sdv_pcm_resample(eng, src.ctypes.data, b - a, 1 if last else 0, out.ctypes.data, cap, C.byref(n_out), None)
            return rc, out[:n_out.value].tobytes()
        return (lambda eng: None), call
    return case


STREAM_CASES = {"audio_process": _audio_process_stream, "audio_deemphasis": _deemphasis_stream, "audio_resample_mode1": _resample_stream(1),
                "audio_resample_mode4": _resample_stream(4), "audio_resample_mode5": _resample_stream(5),
                "pcm_preemphasis": _pcm_stream(False), "pcm_resample": _pcm_stream(True)}


@pytest.mark.parametrize("name", list(STREAM_CASES))
def test_failed_allocation_keeps_the_stream(name, emu_lib):
    setup, call = STREAM_CASES[name](emu_lib)
    spans = list(zip(STREAM_CUTS[:-1], STREAM_CUTS[1:]))

    def stream(fail_call=None, nth=0):
        """The stream on a fresh engine -> (its bytes, the allocations of every call); with `fail_call`: allocation `nth` of that call fails, the call is
        made again."""
        eng = emu_lib.sdv_engine_create(0)
        setup(eng)
        got, allocs = [], []
        for i, (a, b) in enumerate(spans):
            last = i == len(spans) - 1
            if i == fail_call:
                emu_lib.sdv_emu_fail_alloc(nth)
                rc, _ = call(eng, a, b, last)
                left = emu_lib.sdv_emu_fail_alloc(0)
                assert left == 0, f"call {i}: allocation {nth} was never asked for"
                assert rc == SDV_ERR_HIP, f"call {i}: allocation {nth} failed and the call returned {rc}"
            emu_lib.sdv_emu_fail_alloc(FAR)
            rc, out = call(eng, a, b, last)
            allocs.append(FAR - emu_lib.sdv_emu_fail_alloc(0))
            assert rc == 0, f"call {i}{' repeated after a failure at allocation %d' % nth if i == fail_call else ''}: {emu_lib.sdv_last_error(eng)}"
            got.append(out)
        emu_lib.sdv_engine_destroy(eng)
        return b"".join(got), allocs

    want, allocs = stream()
    assert allocs[0] >= 1, "the first call allocates nothing?"
    for i, n_allocs in enumerate(allocs):
        for k in range(1, n_allocs + 1):
            got, _ = stream(i, k)
            assert got == want, f"after a failure at allocation {k} of {n_allocs} in call {i} the stream differs from the clean run"
