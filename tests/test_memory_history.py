"""No result may depend on what memory held before the call (the stages, their compact cases and the three properties: tests/memory_history.py).

  (a) poisoned allocations   every buffer the engines allocate is prefilled with 0x55, then with 0xFF: a counter, flag, offset or bitmap word that is read
                             before anything wrote it no longer finds the zero a fresh engine in a young process usually gets
  (b) an engine with a past  a larger case with other settings, the stage's start-over entry, then the compact cases forwards and backwards on one engine:
                             the buffers are larger than the case needs and hold another tape's plausible records
  (c) dirty caller buffers   (b) runs through output buffers that start as 0xA5 bytes: a record or a padding byte a kernel believes is already clear
                             fails the byte comparison with the reference

on the SIMT emulator (CPU) and on the GPU (-m gpu).  The emulator runs the same host code and kernel bodies, in order on one stream; what it cannot show -
concurrent host paths, side streams, buffers written ahead, launches at estimated widths, real launch geometry - is what the GPU twins are for.  On the
GPU (a) runs the developer build of the HIP library (SDV_POISON_ALLOC; the product library reads no environment) in a process of its own."""
import numpy as np
import pytest

import device_calls as dc
import memory_history as mh

FAR = 1 << 30


def _lib(emu_lib):
    """the emulator build, or with None the product library, bound with every prototype"""
    return dc.product_lib() if emu_lib is None else dc.emu_lib_of(emu_lib)


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------------------------
def _poisoned_allocations(emu_lib, names):
    if emu_lib is not None:
        lib = _lib(emu_lib)
        for name in names:
            for byte in mh.POISON_BYTES:
                prev = lib.sdv_emu_poison_alloc(byte)
                try:
                    mh.run_fresh(lib, mh.memory("host"), name)
                finally:
                    was = lib.sdv_emu_poison_alloc(prev)
                assert was == byte, "the poison byte was %d when the stage had run, not %d" % (was, byte)
        return
    # the GPU: a child per byte, the second one only behind a clean first one
    for byte in mh.POISON_BYTES:
        status, filled, peeks, output = mh.gpu_child(byte, names, timeout=420)
        assert status == 0 and "HISTORY_OK" in output, "under 0x%02X: exit status %d\n%s" % (byte, status, output)
        assert sorted(p["pinned"] for p in peeks) == [0, 1] and all(p["all"] for p in peeks), peeks      # the fill lands in device and in pinned memory
        assert list(filled) == list(names)
        empty = [name for name in names if filled[name][0] < 1 or filled[name][1] < 1]
        assert not empty, "nothing was filled for %s: the stage allocates nothing under the hook (a bug of this test)" % empty


@pytest.mark.parametrize("name", mh.POISONED_STAGES)
def test_emu_poisoned_allocations(name, emu_lib, oracle_lib):
    _poisoned_allocations(emu_lib, [name])


@pytest.mark.gpu
def test_gpu_poisoned_allocations(oracle_lib):
    _poisoned_allocations(None, mh.POISONED_STAGES)


def test_stages_without_engine_memory_allocate_nothing(emu_lib, oracle_lib):
    """The stages left out of (a) are the ones that own no memory: counted, not assumed - and every other stage allocates."""
    lib = _lib(emu_lib)
    for name, stage in mh.STAGES.items():
        lib.sdv_emu_fail_alloc(FAR)
        try:
            mh.run_fresh(lib, mh.memory("host"), name)
        finally:
            n = FAR - lib.sdv_emu_fail_alloc(0)
        assert (n > 0) == stage.allocates, "%s made %d allocations" % (name, n)


# ---- (b) and (c) ---------------------------------------------------------------------------------------------------------------------------------------
def _engine_with_a_past(emu_lib, name):
    mh.run_with_a_past(_lib(emu_lib), mh.memory("host" if emu_lib is not None else "device", dirty=True), name)


@pytest.mark.parametrize("name", list(mh.STAGES))
def test_emu_engine_with_a_past(name, emu_lib, oracle_lib):
    _engine_with_a_past(emu_lib, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(mh.STAGES))
def test_gpu_engine_with_a_past(name, oracle_lib):
    _engine_with_a_past(None, name)


def _formats_on_one_engine(emu_lib):
    mh.run_formats_on_one_engine(_lib(emu_lib), mh.memory("host" if emu_lib is not None else "device", dirty=True))


def test_emu_formats_on_one_engine(emu_lib, oracle_lib):
    _formats_on_one_engine(emu_lib)


@pytest.mark.gpu
def test_gpu_formats_on_one_engine(oracle_lib):
    _formats_on_one_engine(None)


# ---- the dirty memories do what they say --------------------------------------------------------------------------------------------------------------
def test_dirty_host_buffers_start_as_the_pattern_and_come_back_overwritten(emu_lib, oracle_lib):
    """Host(dirty=True) hands out 0xA5 bytes; sdv_stitch_frames overwrites every byte of the n_out records it counts (they are the oracle's, padding
    included) and nothing behind them.  The default stays zeros, on both memories."""
    import stitch_api as sa
    lib = _lib(emu_lib)
    recs, st, want = mh._stitch_case("ntsc_bad10_no_pq")
    seen = []

    class Spy(dc.Host):
        def zeros(self, n, dtype, full=None):
            b = dc.Host.zeros(self, n, dtype, full)
            assert b.dtype == np.dtype(dtype) and len(b) == n and (b.view(np.uint8) == dc.PATTERN).all()
            seen.append(b)
            return b

    eng = lib.sdv_engine_create(0)
    rc, pairs, frames = dc.Calls(Spy(dirty=True)).stitch(lib, eng, recs, st)
    lib.sdv_engine_destroy(eng)
    assert rc == 0 and [b.dtype for b in seen] == [sa.PAIR_DTYPE, sa.FRASM_DTYPE]
    for buf, got, ref in zip(seen, (pairs, frames), want):
        assert 0 < len(got) == len(ref) < len(buf)
        assert buf[:len(ref)].tobytes() == ref.tobytes() and (buf[len(ref):].view(np.uint8) == dc.PATTERN).all()
    assert not dc.Host().zeros(5, np.uint32).any() and not dc.Host().dirty and not dc.Device().dirty
    dirty, clean = dc.DevBuf(4, np.uint32, full=6, device="cpu", dirty=True), dc.DevBuf(4, np.uint32, full=6, device="cpu")
    assert dirty.get().view(np.uint8).tolist() == [dc.PATTERN] * 16 and clean.get().tolist() == [0] * 4
    assert dc.Device(dirty=True).dirty
