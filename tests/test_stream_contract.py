"""The stream and device contract of the C-ABI (include/sdvpcm.h): every hot entry point does all its device work on the stream it is given,
"asynchronous on `stream`" and "returns when the outputs are complete" mean what they say, every entry point runs on its engine's device and
restores the caller's, and engines share no device state.  Every other test passes the default stream, where a launch, copy or memset on the
wrong stream cannot show; here every call goes to a non-blocking side stream that is busy, with the input buffer still holding another tape.

Audit of the entry points (read from the code, sdvpcmdecoder_amd/csrc/*.inc):

  entry point                                   stream  device work                         on return      SDV_ON_DEVICE
  sdv_engine_create                             -       probes the device                   -              a DeviceGuard of its own
  sdv_engine_destroy                            -       frees buffers, streams, events      -              a DeviceGuard of its own
  sdv_last_error, sdv_abi_version, sdv_default_bin_preset / _deint_settings / _stitch_settings / _pcm1_stitch_settings /
  _pcm16x0_stitch_settings, sdv_set_bin_preset, sdv_set_mode, sdv_set_check_line_dup, sdv_set_pcm_type, sdv_reset_stream,
  sdv_get / set_chain_state, sdv_pcm16x0_chain_state_size, sdv_get / set_pcm16x0_chain_state, sdv_get_run_info, sdv_set_profiling,
  sdv_set_frame_flags (host copy; the frame entry uploads it on its stream), sdv_needs_double_width, sdv_records_per_frame,
  sdv_binarize_records, sdv_pcm16x0_binarize_records, sdv_set_stitch_settings, sdv_stitch_state_size, sdv_saturate_stitch_stats,
  sdv_set_stitch_block_output / _line_output (store the caller's pointer), sdv_stitch_block_count / _line_count / _line_counts,
  sdv_set_pcm1_stitch_settings, sdv_set_pcm1_stitch_block_output / _line_output, sdv_pcm1_stitch_block_count / _line_count,
  sdv_set_pcm16x0_stitch_settings, sdv_pcm16x0_stitch_state_size, sdv_set_pcm16x0_stitch_block_output / _line_output,
  sdv_pcm16x0_stitch_block_count / _line_count, sdv_set_audio_masking, sdv_reset_audio, sdv_audio_pending / _stalled / _next_index,
  sdv_wav_header, sdv_deemphasis_coeffs, sdv_set_deemphasis, sdv_reset_deemphasis, sdv_vis_canvas_size
                                                -       none (host state only)              -              not needed
  sdv_double_width                              yes     one launch                          asynchronous   direct
  sdv_binarize_frames                           yes     rounds of launches, read-backs      complete       direct
  sdv_binarize_lines                            yes     passes + sweeps, read-backs         complete       direct
  sdv_pcm1_binarize_lines                       yes     memset + launches                   asynchronous   direct
  sdv_pcm16x0_binarize_lines                    yes     one launch                          asynchronous   direct (the header said nothing: added)
  sdv_pcm1_binarize_frames                      yes     rounds of launches, read-backs      complete       markerless_binarize_frames
  sdv_pcm16x0_binarize_frames                   yes     rounds of launches, read-backs      complete       markerless_binarize_frames
  sdv_deinterleave_blocks                       yes     one launch                          asynchronous   direct
  sdv_stitch_frames                             yes     launches, read-backs                complete       stitch_frames_impl
  sdv_get_stitch_info                           -       a read-back on stream 0 when owed   complete       direct, around that read-back
  sdv_reset_stitcher                            -       h2d + sync on stream 0              complete       WAS MISSING - added
  sdv_get_stitch_state                          -       d2h on stream 0                     complete       WAS MISSING - added
  sdv_set_stitch_state                          -       hipMalloc, h2d + sync on stream 0   complete       WAS MISSING - added
  sdv_pcm1_stitch_frames                        yes     launches, read-backs                complete       direct
  sdv_pcm1_bin_to_line_recs                     yes     one launch                          asynchronous   direct
  sdv_get / set_pcm16x0_stitch_state            -       d2h / hipMalloc, h2d on stream 0    complete       direct
  sdv_saturate_pcm16x0_stitch_stats             -       through the two above               complete       through them
  sdv_pcm16x0_stitch_frames                     yes     launches on `stream` and on three private streams forked and joined by events    complete    direct
  sdv_audio_process                             yes     launches, read-backs                complete       direct
  sdv_wav_pack                                  yes     one launch                          asynchronous   direct
  sdv_audio_deemphasis                          yes     two launches (or a d2d copy)        asynchronous   direct
  sdv_decode_frames                             yes     the stages above                    complete, but for the de-emphasis pass when one is set (added to the header)    direct, and again in every stage
  sdv_vis_reset                                 yes     one launch                          asynchronous   direct (the header said nothing: added)
  sdv_vis_render_lines                          yes     launches, one read-back             the frame count is read back, the drawing is asynchronous    direct
  sdv_vis_render_blocks, sdv_vis_render_asm_lines   yes launches, one h2d + sync            asynchronous   vis_render_rows

The scenario table is tests/stream_scenarios.py; the CPU twins drive it through the emulator build (which ignores the stream) so that the
tapes, the shapes, the expected bytes and the "tape A and tape B decode differently" precondition are checked without a GPU."""
import ctypes as C

import numpy as np
import pytest

import stream_scenarios as ss
from stream_scenarios import SCENARIOS, PCM1, PCM16X0, STC007, VP, ok

COMPLETE = [s for s in SCENARIOS if s.complete]
BUSY_BYTES = 256 << 20      # the unrelated work in front of every streamed call: four fills of this much


def check(outs, want, fetch):
    assert len(outs) == len(want)
    for i, (o, w) in enumerate(zip(outs, want)):
        got = o if isinstance(o, np.ndarray) else fetch(o)
        assert ss.as_bytes(got).tobytes() == ss.as_bytes(w).tobytes(), "output %d differs from the oracle's (%d bytes for %d)" % (i, ss.as_bytes(got).size, ss.as_bytes(w).size)


# ---- the emulator build: host memory, no streams ----------------------------------------------------------------------------------------------
class HostCtx:
    s = None

    def __init__(self, lib):
        self.lib, self.engines = ss.bind(lib), []

    def engine(self):
        h = VP(self.lib.sdv_engine_create(0))
        assert h
        self.engines.append(h)
        return h

    def reserve_engines(self, n):
        pass

    def ptr(self, a):
        return a.ctypes.data

    def out(self, n):
        return np.zeros(max(n, 1), dtype=np.uint8)

    def stage(self, a, b):
        return ss.as_bytes(a).copy()

    def copy_in(self, buf):
        pass

    def cat(self, parts):
        return np.concatenate([b[lo:hi] for b, lo, hi in parts])

    def close(self):
        for h in self.engines:
            self.lib.sdv_engine_destroy(h)


def host_fetch(o):
    return o[0][:o[1]]


@pytest.mark.parametrize("sc", SCENARIOS, ids=repr)
def test_cpu_tapes_decode_differently(sc, oracle_lib):
    """The precondition of the stale-input scenario: what the oracle makes of tape B is not what it makes of tape A, record for record, so an
    engine that read tape B, or half of each, cannot pass.  Every record that carries something of the tape differs (stream_scenarios.KINDS
    says which do: all but service lines, file tags and pairs that are silent on both tapes), and those are most of every output."""
    inp_a, want_a = sc.made("A")
    inp_b, want_b = sc.made("B")
    assert len(want_a) == len(want_b) == len(sc.kinds)
    for k in inp_a:
        if not k.startswith("_"):
            assert ss.as_bytes(inp_a[k]).tobytes() != ss.as_bytes(inp_b[k]).tobytes()
    for i, (wa, wb, kind) in enumerate(zip(want_a, want_b, sc.kinds)):
        if kind in ss.POSITIONAL:
            continue
        carry, differ, n = ss.tape_records(kind, wa, wb)
        print("%s output %d (%s): %d of %d records carry the tape, %d of them differ" % (sc.name, i, kind, carry, n, differ))
        assert n > 0 and differ == carry and 2 * carry > n, (i, kind, carry, differ, n)


@pytest.mark.parametrize("sc", SCENARIOS, ids=repr)
def test_cpu_twin(sc, emu_lib, oracle_lib):
    inp, want = sc.made("A")
    ctx = HostCtx(emu_lib)
    try:
        dev = {k: ss.as_bytes(v).copy() for k, v in inp.items() if not k.startswith("_")}
        check(sc.run(ctx, dev, inp), want, host_fetch)
    finally:
        ctx.close()


# ---- the state entry points between two halves of a tape; two engines side by side (shared by the CPU twins and the GPU tests) -----------------
def halves_of(fmt):
    """(frames per half, frames per call): the STC-007 halves go in two calls each, so that a second call finds a stitcher that plays (three
    frame segments with the one that waited: the pipelined path of sdv_stitch_frames) and the state is exported behind such a call."""
    return (4, 2) if fmt == STC007 else (3, 3)


def handover_tape(fmt, tape):
    half, _ = halves_of(fmt)
    if fmt == STC007:
        return ss.stc_tape(tape, 2 * half, 12)
    return ss.pcm_tape(fmt, tape, 2 * half)


def frames_of(fmt):
    return {STC007: ("sdv_binarize_frames", 48, 1), PCM1: ("sdv_pcm1_binarize_frames", 40, 1), PCM16X0: ("sdv_pcm16x0_binarize_frames", 36, 3)}[fmt]


def stitch_half(ctx, h, fmt, recs, n_recs):
    if fmt == STC007:
        return ss.call_stitch(ctx, h, "sdv_stitch_frames", recs, n_recs, 64, 8)
    if fmt == PCM1:
        lines = ctx.out(n_recs * 32)
        ok(ctx, h, ctx.lib.sdv_pcm1_bin_to_line_recs(h, ctx.ptr(recs), n_recs, ctx.ptr(lines), ctx.s))
        return ss.call_stitch(ctx, h, "sdv_pcm1_stitch_frames", lines, n_recs, 52, 6)
    return ss.call_stitch(ctx, h, "sdv_pcm16x0_stitch_frames", recs, n_recs, 56, 6)


def blob(lib, h, size, get):
    buf = C.create_string_buffer(size)
    assert get(h, buf, size) == 0, lib.sdv_last_error(h)
    return buf


def handover(ctx1, ctx2, fmt):
    """First half on engine 1 / stream 1, its states into a fresh engine 2, the second half at once on stream 2 -> (pairs, frames) per call."""
    lib = ctx1.lib
    half, step = halves_of(fmt)
    luma_a, luma_b = handover_tape(fmt, "A"), handover_tape(fmt, "B")
    _, hgt, w = luma_a.shape
    fn, rec_bytes, per_row = frames_of(fmt)
    per_frame = per_row * hgt + 3
    ctxs = (ctx1, ctx2)
    bufs = [[ctxs[k].stage(luma_a[k * half + c:k * half + c + step], luma_b[k * half + c:k * half + c + step]) for c in range(0, half, step)] for k in (0, 1)]
    ctx1.reserve_engines(1)
    ctx2.reserve_engines(1)
    ctx1.staged()
    ctx2.staged()
    outs, piped, last_recs = [], [], None
    eng = []
    for k in (0, 1):
        ctx = ctxs[k]
        e = ctx.engine()
        eng.append(e)
        ok(ctx, e, lib.sdv_set_pcm_type(e, fmt, 0))
        if k == 1:
            e1 = eng[0]
            if fmt == PCM16X0:
                chain = blob(lib, e1, lib.sdv_pcm16x0_chain_state_size(), lib.sdv_get_pcm16x0_chain_state)
                state = blob(lib, e1, lib.sdv_pcm16x0_stitch_state_size(), lib.sdv_get_pcm16x0_stitch_state)
                assert lib.sdv_set_pcm16x0_chain_state(e, chain, len(chain)) == 0 and lib.sdv_set_pcm16x0_stitch_state(e, state, len(state)) == 0, lib.sdv_last_error(e)
            else:
                chain = C.create_string_buffer(120)
                assert lib.sdv_get_chain_state(e1, chain) == 0 and lib.sdv_set_chain_state(e, chain) == 0
                if fmt == STC007:
                    state = blob(lib, e1, lib.sdv_stitch_state_size(), lib.sdv_get_stitch_state)
                    assert lib.sdv_set_stitch_state(e, state, len(state)) == 0, lib.sdv_last_error(e)
        ctx.busy()
        for c, buf in enumerate(bufs[k]):
            ctx.copy_in(buf)
            first, last = k == 0 and c == 0, k == 1 and c + 1 == len(bufs[k])
            n_recs = step * per_frame + (1 if first else 0) + (hgt + 4 if last else 0)
            recs, _ = ss.call_frames(ctx, e, fn, buf, (step, hgt, w), 1 + k * half + c * step, (1 if first else 0) | (4 if last else 0), rec_bytes, n_recs, step + (1 if last else 0))
            if fmt == STC007 and k == 1 and c == 0:
                # the frame that waited in engine 1 for its successor is not part of the state (sdvpcm.h): its records go in again, in front of the second half's
                lo = last_recs[1] - per_frame * rec_bytes
                both = ctx.cat([(last_recs[0], lo, last_recs[1]), (recs[0], 0, n_recs * rec_bytes)])
                outs += stitch_half(ctx, e, fmt, both, per_frame + n_recs)
            else:
                outs += stitch_half(ctx, e, fmt, recs[0], n_recs)
            if fmt == STC007:
                piped.append(int(ss.stitch_info(ctx, e).pipelined))
            last_recs = recs
    if fmt == STC007:
        # engine 1's second call took the path of a stream that plays, from the state its first call left; engine 2's second call ends the file
        # (filler frame and END_FILE tag), which that path does not take
        assert piped[1], piped
    return outs


def handover_check(outs, fmt, orc, fetch):
    pairs, frames, _ = ss.oracle_chain(orc, fmt, handover_tape(fmt, "A"), 1)
    got = [ss.as_bytes(fetch(o)) for o in outs]
    assert np.concatenate(got[0::2]).tobytes() == ss.as_bytes(pairs).tobytes(), "sample pairs differ from the oracle's sequential decode"
    assert np.concatenate(got[1::2]).tobytes() == ss.as_bytes(frames).tobytes(), "frame descriptors differ from the oracle's sequential decode"
    assert len(got[0]) > 0 and len(got[-2]) > 0


TURNS, TURN_FRAMES = 3, 2      # (a first call of two frames is one stitcher turn: the second call can assume its layout)


def two_engine_tapes():
    return [ss.stc_tape("A", TURNS * TURN_FRAMES, 12), ss.stc_tape("B", TURNS * TURN_FRAMES, 57)]


def two_engines(ctx1, ctx2):
    """Two tapes, two frames per turn, frames -> stitch -> audio on two engines in turns, each on its own stream
    -> per engine (pairs, frames, purges) of every turn, then the masked count and the pairs every stitch call made."""
    import audio_api as au
    import stitch_api as sa
    ctxs, tapes = (ctx1, ctx2), two_engine_tapes()
    n, hgt, w = tapes[0].shape
    bufs = [[ctxs[i].stage(tapes[i][k:k + TURN_FRAMES], tapes[1 - i][k:k + TURN_FRAMES]) for k in range(0, n, TURN_FRAMES)] for i in (0, 1)]
    ctx1.reserve_engines(1)
    ctx2.reserve_engines(1)
    ctx1.staged()
    ctx2.staged()
    eng = []
    for ctx in ctxs:
        h = ctx.engine()
        st = sa.default_settings()
        ok(ctx, h, ctx.lib.sdv_set_stitch_settings(h, C.byref(st)))
        ok(ctx, h, ctx.lib.sdv_set_audio_masking(h, au.DROP_INTER_LIN_WORD))
        eng.append(h)
    outs, masked, bursts, piped = [[], []], [0, 0], [[], []], []
    for i in (0, 1):
        ctxs[i].busy()
    for t in range(TURNS):
        first, last = t == 0, t + 1 == TURNS
        n_recs = TURN_FRAMES * (hgt + 3) + (1 if first else 0) + (hgt + 4 if last else 0)
        for i in (0, 1):
            ctxs[i].copy_in(bufs[i][t])
        recs = [ss.call_frames(ctxs[i], eng[i], "sdv_binarize_frames", bufs[i][t], (TURN_FRAMES, hgt, w), 1 + t * TURN_FRAMES, (1 if first else 0) | (4 if last else 0),
                               48, n_recs, TURN_FRAMES + (1 if last else 0)) for i in (0, 1)]
        raw = [ss.call_stitch(ctxs[i], eng[i], "sdv_stitch_frames", recs[i][0][0], n_recs, 64, TURN_FRAMES + 3) for i in (0, 1)]
        piped += [int(ss.stitch_info(ctxs[i], eng[i]).pipelined) for i in (0, 1)]
        for i in (0, 1):
            ctx, h = ctxs[i], eng[i]
            n_pairs = raw[i][0][1] // 12
            cap = n_pairs + 1024
            out, pur = ctx.out(cap * 12), ctx.out(8 * 16)
            n_out, n_pur, nm = C.c_size_t(0), C.c_size_t(0), C.c_uint64(0)
            ok(ctx, h, ctx.lib.sdv_audio_process(h, ctx.ptr(raw[i][0][0]), n_pairs, 1 if last else 0, ctx.ptr(out), cap, C.byref(n_out), ctx.ptr(pur), 8, C.byref(n_pur), C.byref(nm), ctx.s))
            outs[i] += [(out, n_out.value * 12), raw[i][1], (pur, n_pur.value * 16)]
            masked[i] += nm.value
            bursts[i].append(n_pairs)
    assert any(piped[2:]), piped            # the later turns took the stitcher's path of a stream that plays
    return [outs[i] + [np.array([masked[i]], dtype=np.uint64), np.array(bursts[i], dtype=np.uint64)] for i in (0, 1)]


def two_engines_check(outs, orc, fetch):
    import audio_api as au
    for i, luma in enumerate(two_engine_tapes()):
        pairs, frames, _ = ss.oracle_chain(orc, STC007, luma, 1)
        bursts = outs[i][-1]
        assert int(bursts.sum()) == len(pairs)      # (how the pairs came call by call is the AudioProcessor's feed schedule; what they are is the oracle's)
        w_out, _, w_pur, w_masked, hit = au.run_cpu(orc, "orc_", pairs, au.DROP_INTER_LIN_WORD, np.cumsum(bursts).astype(np.uint64), 1)
        assert hit == 0
        got = [o if isinstance(o, np.ndarray) else ss.as_bytes(fetch(o)) for o in outs[i][:-2]]
        got_pur = np.concatenate(got[2::3]).view(au.PURGE_DTYPE).copy()
        at, seen = 0, 0
        turn_pur = [len(g) // 16 for g in got[2::3]]
        for t, cnt in enumerate(turn_pur):           # a call counts its purges from its own first pair
            got_pur["first_pair"][at:at + cnt] += seen
            got_pur["tag_index"][at:at + cnt] += int(np.cumsum(bursts)[t - 1]) if t else 0
            at += cnt
            seen += len(got[3 * t]) // 12
        assert np.concatenate(got[0::3]).tobytes() == ss.as_bytes(w_out).tobytes(), "engine %d: masked pairs differ from the oracle's" % i
        assert np.concatenate(got[1::3]).tobytes() == ss.as_bytes(frames).tobytes(), "engine %d: frame descriptors differ from the oracle's" % i
        assert got_pur.tobytes() == ss.as_bytes(w_pur).tobytes() and int(outs[i][-2][0]) == w_masked, "engine %d: purges / masked count differ" % i


class HostCtx2(HostCtx):
    def staged(self):
        pass

    def busy(self):
        pass


@pytest.mark.parametrize("fmt", [STC007, PCM1, PCM16X0], ids=["stc007", "pcm1", "pcm16x0"])
def test_cpu_twin_state_handover(fmt, emu_lib, oracle_lib):
    ctx1, ctx2 = HostCtx2(emu_lib), HostCtx2(emu_lib)
    try:
        handover_check(handover(ctx1, ctx2, fmt), fmt, oracle_lib, host_fetch)
    finally:
        ctx1.close()
        ctx2.close()


def test_cpu_twin_two_engines(emu_lib, oracle_lib):
    ctx1, ctx2 = HostCtx2(emu_lib), HostCtx2(emu_lib)
    try:
        two_engines_check(two_engines(ctx1, ctx2), oracle_lib, host_fetch)
    finally:
        ctx1.close()
        ctx2.close()


# ---- the product on the GPU -------------------------------------------------------------------------------------------------------------------
class GpuCtx:
    """Device memory as torch.uint8 tensors; every call goes to `stream`, a non-blocking stream of `device` that is not the current one."""

    def __init__(self, device=0):
        import torch
        from sdvpcmdecoder_amd import load_library
        torch.cuda.init()
        self.torch, self.lib, self.device, self.engines, self.pending, self.pool = torch, ss.bind(load_library()), device, [], {}, []
        self.ballast = torch.empty(BUSY_BYTES, dtype=torch.uint8, device="cuda:%d" % device)
        self.stream = torch.cuda.Stream(device=device)
        assert self.stream.cuda_stream != 0 and self.stream != torch.cuda.current_stream(device)
        self.s = VP(self.stream.cuda_stream)
        self.here = torch.cuda.current_device() == device      # (with another current device nothing here may switch to the engine's: that is the engine's job)

    def reserve_engines(self, n):
        """Engines made ahead of the work on the stream (what an engine allocates in its first call cannot be: it is part of the call)."""
        for _ in range(n):
            h = VP(self.lib.sdv_engine_create(self.device))
            assert h, self.lib.sdv_last_error(None)
            self.engines.append(h)
            self.pool.append(h)

    def engine(self):
        if not self.pool:
            self.reserve_engines(1)
        return self.pool.pop(0)

    def pending_mark(self):
        """An event behind what is queued on the stream so far: was it still pending when the entry point was called?"""
        ev = self.torch.cuda.Event()
        if self.here:
            ev.record(self.stream)
        return ev

    def ptr(self, t):
        return t.data_ptr()

    def out(self, n):
        return self.torch.empty(max(n, 1), dtype=self.torch.uint8, device="cuda:%d" % self.device)

    def stage(self, a, b):
        """The device buffer of an input, holding tape B (in A's size); A waits in page-locked memory for copy_in."""
        a = ss.as_bytes(a)
        t = self.torch.from_numpy(np.resize(ss.as_bytes(b), a.size).copy()).to("cuda:%d" % self.device)
        self.pending[t.data_ptr()] = self.torch.from_numpy(a.copy()).pin_memory()
        return t

    def staged(self):
        self.torch.cuda.synchronize(self.device)

    def busy(self):
        """A few milliseconds of unrelated work on the stream, so that what follows is still pending when the entry point is called."""
        if self.here:
            with self.torch.cuda.stream(self.stream):
                for v in range(4):
                    self.ballast.fill_(v)

    def copy_in(self, t):
        if self.here:
            with self.torch.cuda.stream(self.stream):
                t.copy_(self.pending[t.data_ptr()], non_blocking=True)
        else:
            t.copy_(self.pending[t.data_ptr()])

    def cat(self, parts):
        if self.here:
            with self.torch.cuda.stream(self.stream):
                return self.torch.cat([b[lo:hi] for b, lo, hi in parts])
        self.stream.synchronize()
        return self.torch.cat([b[lo:hi] for b, lo, hi in parts])

    def clone(self, outs, stream):
        with self.torch.cuda.stream(stream):
            return [o if isinstance(o, np.ndarray) else (o[0][:o[1]].clone(), o[1]) for o in outs]

    def close(self):
        self.torch.cuda.synchronize(self.device)
        for h in self.engines:
            self.lib.sdv_engine_destroy(h)


def gpu_fetch(o):
    return o[0][:o[1]].cpu().numpy()


def stale_input(sc, wait_for_side_stream):
    import torch
    inp, want = sc.made("A")
    inp_b, _ = sc.made("B")
    ctx = GpuCtx()
    try:
        dev = {k: ctx.stage(v, inp_b[k]) for k, v in inp.items() if not k.startswith("_")}
        ctx.reserve_engines(1)
        ctx.staged()
        ctx.busy()
        for t in dev.values():
            ctx.copy_in(t)
        mark = ctx.pending_mark()
        was_pending = not mark.query()
        outs = sc.run(ctx, dev, inp)
        # (recorded, not asserted: whether the copy of tape A was still queued when the scenario started, and whether the stream was still busy behind it)
        print("%s: input copy pending at the call: %s; stream busy after the return: %s" % (sc.name, was_pending, not ctx.stream.query()))
        if wait_for_side_stream:        # the outputs of an asynchronous entry are read on its stream
            outs = ctx.clone(outs, ctx.stream)
            ctx.stream.synchronize()
        else:                           # the call has returned: its outputs are complete, whatever stream reads them
            reader = torch.cuda.Stream()
            outs = ctx.clone(outs, reader)
            reader.synchronize()
        check(outs, want, gpu_fetch)
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("sc", SCENARIOS, ids=repr)
def test_gpu_stale_input(sc, oracle_lib):
    """Tape B in the input buffer, a busy side stream, tape A copied in on that stream, the entry point on that stream, its outputs cloned on
    that stream: any operation of the engine on another stream reads tape B or a half-written buffer."""
    stale_input(sc, True)


@pytest.mark.gpu
@pytest.mark.parametrize("sc", COMPLETE, ids=repr)
def test_gpu_complete_on_return(sc, oracle_lib):
    """... and for the entries that return when their outputs are complete: read on a second stream without waiting for the first."""
    stale_input(sc, False)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [STC007, PCM1, PCM16X0], ids=["stc007", "pcm1", "pcm16x0"])
def test_gpu_state_handover_between_streams(fmt, oracle_lib):
    """sdv_get_* / sdv_set_*_state use stream 0 and wait for it: enough for a consumer on a non-blocking stream, with nothing of the first
    engine in flight - the second half follows at once on another side stream, without a device-wide synchronisation."""
    ctx1, ctx2 = GpuCtx(), GpuCtx()
    try:
        outs = handover(ctx1, ctx2, fmt)
        cut = len(outs) // 2
        outs = ctx1.clone(outs[:cut], ctx1.stream) + ctx2.clone(outs[cut:], ctx2.stream)
        ctx1.stream.synchronize()
        ctx2.stream.synchronize()
        handover_check(outs, fmt, oracle_lib, gpu_fetch)
    finally:
        ctx1.close()
        ctx2.close()


@pytest.mark.gpu
def test_gpu_two_engines_two_streams(oracle_lib):
    """Two engines of one device, two tapes, calls in turns on two side streams with no synchronisation between the turns: static device
    state or a staging buffer shared by the engines would mix the tapes."""
    ctx1, ctx2 = GpuCtx(), GpuCtx()
    try:
        outs = two_engines(ctx1, ctx2)
        outs = [ctx1.clone(outs[0], ctx1.stream), ctx2.clone(outs[1], ctx2.stream)]
        ctx1.stream.synchronize()
        ctx2.stream.synchronize()
        two_engines_check(outs, oracle_lib, gpu_fetch)
    finally:
        ctx1.close()
        ctx2.close()


# ---- the device contract: the caller's current device is 0, the engine's is 1 ---------------------------------------------------------------
def two_devices():
    import torch
    return torch.cuda.is_available() and torch.cuda.device_count() >= 2


def on_device_0():
    import torch
    return torch.cuda.current_device() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("sc", SCENARIOS, ids=repr)
def test_gpu_other_device_streamed_entries(sc, oracle_lib):
    """Every streamed entry point on an engine of device 1, inputs on cuda:1, a side stream of device 1, called with device 0 current: it
    succeeds, decodes what the oracle does and leaves device 0 current."""
    if not two_devices():
        pytest.skip("needs two GPUs")
    import torch
    torch.cuda.set_device(0)
    inp, want = sc.made("A")
    ctx = GpuCtx(device=1)
    try:
        dev = {k: ctx.stage(v, v) for k, v in inp.items() if not k.startswith("_")}
        ctx.staged()
        assert on_device_0()
        outs = sc.run(ctx, dev, inp)
        assert on_device_0()
        ctx.stream.synchronize()
        check(outs, want, gpu_fetch)
        for h in ctx.engines:           # ... also from a call that is refused
            assert ctx.lib.sdv_set_stitch_state(h, C.create_string_buffer(1 << 16), 1 << 16) == -1 and on_device_0()
            assert ctx.lib.sdv_set_pcm16x0_stitch_state(h, C.create_string_buffer(1 << 20), 1 << 20) == -1 and on_device_0()
            assert ctx.lib.sdv_binarize_frames(h, dev[next(iter(dev))].data_ptr(), 720, 720 * 8, 720, 8, 1, 1, 1, ctx.out(48).data_ptr(), 1, ctx.out(32).data_ptr(), 1, ctx.s) == -1
            assert on_device_0()
    finally:
        ctx.close()
        assert on_device_0()            # (sdv_engine_destroy)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [STC007, PCM1, PCM16X0], ids=["stc007", "pcm1", "pcm16x0"])
def test_gpu_other_device_state_entries(fmt, oracle_lib):
    """The state entry points on engines of device 1 with device 0 current - sdv_set_stitch_state on a fresh engine allocates the hand-over
    chain (on the caller's device before the guard was added) - followed by the decode of the second half; then the other entries that touch
    the device without a stream."""
    if not two_devices():
        pytest.skip("needs two GPUs")
    import torch
    torch.cuda.set_device(0)
    ctx1, ctx2 = GpuCtx(device=1), GpuCtx(device=1)
    try:
        outs = handover(ctx1, ctx2, fmt)
        assert on_device_0()
        ctx1.stream.synchronize()
        ctx2.stream.synchronize()
        handover_check(outs, fmt, oracle_lib, gpu_fetch)
        lib = ctx1.lib
        info = ss.ea.StitchInfo()
        for h in ctx1.engines + ctx2.engines:
            assert lib.sdv_reset_stitcher(h) == 0 and on_device_0()
            assert lib.sdv_saturate_pcm16x0_stitch_stats(h) == 0 and on_device_0()
            assert lib.sdv_vis_reset(h, 0, ctx1.s) == 0 and on_device_0()
            assert lib.sdv_get_stitch_info(h, C.byref(info)) in (0, -1) and on_device_0()
            blob(lib, h, lib.sdv_stitch_state_size(), lib.sdv_get_stitch_state)
            assert on_device_0()
    finally:
        ctx1.close()
        ctx2.close()
        assert on_device_0()
