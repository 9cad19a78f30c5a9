"""Cubic interpolation of short dropouts in the audio masking stage: SDV_DROP_INTER_CUBIC_BLOCK / _WORD of sdv_set_audio_masking (include/sdvpcm.h).

The reference has no such mode, so there is no oracle for it.  The definition the kernels are held to is tests/conceal_walk.py, a plain sequential walk of
the stage written from the header's text with the fill as a parameter.  The walk is pinned first: with the linear, hold and mute fills it gives the bytes
of the oracle (which is pinned to the real AudioProcessor) on the existing inputs and on random tapes.  Then:

  parity      the emulator build and the GPU against the walk, bytewise on pairs, purges and n_masked, on layouts chosen for every branch of the rule
  untouched   modes 0..6 before and after a cubic call on the same engine; refusals
  purpose     on a tone, mode 9 stays within the interpolant's own error, which mode 6 misses by far
  arithmetic  the integer formula: weights sum to D, cubics are reproduced exactly, 32 bits suffice

Positions: in a file that opens with NEW_FILE and holds only short runs that a scan repairs, the windows start 509 pairs apart; with the silent pair of the
purge as pair 0, window k holds the pairs 509 k .. 509 k + 511 (it puts out the first 509, three stay), so entry e of window k is data pair 509 k + e - 1.
test_walk_windows_follow_the_closed_form holds the walk to that, independently of how it counts."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest

import audio_api as A
import conceal_walk as W
import device_calls as dc
from sdvpcmdecoder_amd import abi
from stitch_api import PAIR_DTYPE

CUBIC_WORD, CUBIC_BLOCK = abi.DROP_INTER_CUBIC_WORD, abi.DROP_INTER_CUBIC_BLOCK
LIN_OF = {CUBIC_WORD: A.DROP_INTER_LIN_WORD, CUBIC_BLOCK: A.DROP_INTER_LIN_BLOCK}
STRIDE = W.WIN - W.KEEP


def at(k, e):
    """the data pair that is entry e of window k (see the module's text)"""
    return STRIDE * k + e - 1


def _diff(out, want):
    n = min(len(out), len(want))
    d = np.nonzero((out[:n].view(np.uint8).reshape(n, 12) != want[:n].view(np.uint8).reshape(n, 12)).any(axis=1))[0]
    return f"pairs {len(out)} vs {len(want)}; {len(d)} differ, first at {d[:8]}: got {out[d[:3]]} want {want[d[:3]]}"


# ---- the walk is pinned ---------------------------------------------------------------------------------------------------------------------------------
PIN_INPUTS = ("short_runs_lin", "window_edges", "bursts_long_runs", "worn_tape", "two_files", "no_first_tag", "tiny_files_bad")
PIN_FILLS = {"lin": (A.DROP_INTER_LIN_WORD, W.fill_lin), "hold": (A.DROP_HOLD_WORD, W.fill_hold), "mute": (A.DROP_MUTE_WORD, W.fill_mute)}


@pytest.mark.parametrize("fill", sorted(PIN_FILLS))
@pytest.mark.parametrize("name", PIN_INPUTS)
def test_walk_equals_the_oracle(name, fill, oracle_lib):
    pairs, _, ends, stop = A.make_input(name)
    mode, f = PIN_FILLS[fill]
    want, _, want_pur, want_masked, _ = A.run_cpu(oracle_lib, "orc_", pairs, mode, ends, stop)
    out, pur, masked, _ = W.run(pairs, mode, ends, stop, fill=f)
    assert out.tobytes() == want.tobytes(), _diff(out, want)
    assert pur.tobytes() == want_pur.tobytes() and masked == want_masked


def test_walk_equals_the_oracle_on_random_tapes(oracle_lib):
    """40 seeds of tools/audio_fuzz.py's generator: files, runs, blocks, foreign masked flags, tags in any order, bursts, every mode 0..6."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("audio_fuzz", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "audio_fuzz.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    for seed in range(9000, 9040):
        pairs, mode, ends, stop = fz.random_case(seed)
        want, _, want_pur, want_masked, _ = A.run_cpu(oracle_lib, "orc_", pairs, mode, ends, stop)
        out, pur, masked, _ = W.run(pairs, mode, ends, stop)
        assert out.tobytes() == want.tobytes() and pur.tobytes() == want_pur.tobytes() and masked == want_masked, (seed, mode, list(ends), stop)


# ---- arithmetic ---------------------------------------------------------------------------------------------------------------------------------------------
def test_cubic_weights_sum_to_the_denominator_and_fit_32_bits():
    worst, biggest = 0, 0
    for L in range(2, abi.AP_CUBIC_MAX_RUN + 2):
        D = L * (L + 1) * (L + 2)
        for t in range(1, L):
            c = W.cubic_coeffs(L, t)
            assert sum(c) == D
            biggest = max(biggest, max(abs(x) for x in c))
            for v in (-32768, 32767):           # the extreme of N: every node at full scale with the sign of its weight, or against it
                N = sum(x * (v if x > 0 else -v - 1) for x in c)
                worst = max(worst, abs(2 * N + D))
    assert biggest < 1848 and worst < 2 ** 31
    assert W.cubic_coeffs(2, 1) == (-4, 16, 16, -4)         # a single missing sample: (-vp + 4 va + 4 vb - vq) / 6 over D = 24


def test_cubic_formula_reproduces_integer_cubics():
    rng = np.random.default_rng(3)
    for L in range(2, abi.AP_CUBIC_MAX_RUN + 2):
        for _ in range(50):
            k = [int(x) for x in rng.integers(-20, 21, 4)]
            f = lambda x: k[0] + k[1] * x + k[2] * x * x + k[3] * x * x * x
            for t in range(1, L):
                assert W.cubic_value(L, t, f(-1), f(0), f(L), f(L + 1)) == f(t), (L, t, k)
    assert W.cubic_value(2, 1, -32768, 32767, 32767, -32768) == 32767 and W.cubic_value(2, 1, 32767, -32768, -32768, 32767) == -32768     # 54 612, clamped
    assert W.cubic_value(2, 1, 1, 1, 0, 0) == 1 and W.cubic_value(2, 1, -1, -1, 0, 0) == 0                  # N / D = 12 / 24 and -12 / 24: halves go up


# ---- the layouts -----------------------------------------------------------------------------------------------------------------------------------------
def _noise(n, seed, runs=(), tone=False):
    return A.audio(n, seed, runs=list(runs), tone=tone)


def _c_singles_noise():
    return A.tape(["N", _noise(3000, 101, [(200, 1, 0), (333, 1, 1), (700, 1, 2), (1201, 1, 0), (1204, 1, 1), (2222, 1, 2), (2224, 1, 0)]), "E"]), None


def _c_singles_tone():
    return A.tape(["N", _noise(3000, 102, [(150, 1, 1), (400, 1, 0), (640, 1, 2), (1500, 1, 1), (1503, 1, 0), (2100, 1, 2)], tone=True), "E"]), (0.2, 0.21, 0.7, 1.0)


def _c_runs_1_to_8():
    runs = [(200 + 100 * ln, ln, ln % 2) for ln in range(1, 9)] + [(1500 + 100 * ln, ln, 2) for ln in range(1, 9)]
    return A.tape(["N", _noise(2600, 103, runs, tone=True), "E"]), None


def _c_v_i_v_i_v():
    return A.tape(["N", _noise(1500, 104, [(300, 1, 0), (302, 1, 0), (600, 1, 2), (602, 1, 2), (604, 1, 2), (900, 1, 0)], tone=True), "E"]), None


def _c_outer_filled_earlier():
    # entry 509 of window 1 is filled by that scan; the run at entry 511 waits for window 2, where the filled sample is its lower outer neighbour
    return A.tape(["N", _noise(2000, 105, [(at(1, 509), 1, 0), (at(1, 511), 1, 0), (at(2, 40), 1, 0)], tone=True), "E"]), None


def _c_above_is_last_entry():
    return A.tape(["N", _noise(3200, 106, [(at(2, 510), 1, 1), (at(4, 509), 1, 1)], tone=True), "E"]), None


def _c_behind_the_kept_pairs():
    # the first data pair of the file (entry 1: nothing below its lower neighbour) and the second (the silent pair is its outer neighbour); entry 1 of window 2,
    # which window 1 fills as its entry 510; runs that start at entry 3.  (Entries 0 .. 2 of a later window were scanned by the one before, but for a run at its
    # entry 511, which waits and is entry 3 of the next window: outer_filled_earlier.)
    return A.tape(["N", _noise(3200, 107, [(0, 1, 0), (1, 1, 1), (at(2, 1), 1, 0), (at(4, 3), 2, 2), (at(5, 3), 6, 1)], tone=True), "E"]), None


N_CHAINS = 66


def _overlap_chain_raw():
    """Pairs of windows (2 j + 1, 2 j + 2) that hang together: entries 508 and 510 of the first are invalid, and entry 3 of the second (the overlap of the two is
    the first one's entries 509 .. 511).  What the first window makes of entry 510 decides what the second reads at its entry 1."""
    runs = []
    for j in range(N_CHAINS):
        k, ch = 2 * j + 1, j % 2
        runs += [(at(k, 508), 1, ch), (at(k, 510), 1, ch), (at(k + 1, 3), 1, ch)]
    return A.tape(["N", _noise(STRIDE * (2 * N_CHAINS + 2) + 100, 108, runs, tone=True), "E"]), runs


def _c_overlap_chain():
    """... and the invalid word at entry 510 already holds the value its scan gives it: it comes out valid and not masked, so in the second window it qualifies
    as the outer neighbour of the run at entry 3 - but only once the first window has been worked on.  A second window that ran ahead of its first one would
    find it invalid and draw a line (and a first window that ran behind its second one would find entry 510 valid and take it for a cubic's outer node)."""
    pairs, runs = _overlap_chain_raw()
    out, _, _, w = W.run(pairs, CUBIC_WORD, [len(pairs)], 1)
    for s, _, ch in runs[1::3]:
        pairs["audio_word"][s + 1, ch] = out["audio_word"][np.flatnonzero(w.out_gids == s + 1)[0], ch]       # (+ 1: the NEW_FILE tag)
    return pairs, None


def _c_long_runs_and_file_ends():
    a = _noise(4000, 23, [(250, 900, 0), (1300, 20, 0), (1500, 1000, 1), (2600, 40, 2)], tone=True)        # a window that ends inside a run: `altered` starts
    b = _noise(2500, 8, [(700, 225, 1), (1200, 230, 0), (2300, 200, 2)], tone=True)                       # ramps, and a file that ends in invalid samples
    return A.tape(["N", a, "E", "N", b, "E"]), (0.13, 0.5, 0.51, 0.9, 1.0)


def _c_blocks():
    return A.tape(["N", A.audio(4000, 7, p_block=0.03, p_bad=0.005), "E"]), None


def _c_full_scale():
    a = _noise(1200, 109)
    for s, five in ((300, (-32768, 32767, 1234, 32767, -32768)), (700, (32767, -32768, 1234, -32768, 32767)),      # 54 612 / -54 613: clamped
                    (500, (1, 1, 77, 0, 0)), (900, (-1, -1, 77, 0, 0))):                                         # N / D = 1 / 2 and -1 / 2: halves go up
        for ch in range(2):
            a["audio_word"][s - 2:s + 3, ch] = five
        a["sample_flags"][s - 2:s + 3] = A.SF_BLOCK_OK | A.SF_WORD_VALID
        a["sample_flags"][s] = A.SF_BLOCK_OK
    return A.tape(["N", a, "E"]), None


LAYOUTS = {"singles_noise": _c_singles_noise, "singles_tone": _c_singles_tone, "runs_1_to_8": _c_runs_1_to_8, "v_i_v_i_v": _c_v_i_v_i_v,
           "outer_filled_earlier": _c_outer_filled_earlier, "above_is_last_entry": _c_above_is_last_entry, "behind_the_kept_pairs": _c_behind_the_kept_pairs,
           "overlap_chain": _c_overlap_chain, "long_runs_and_file_ends": _c_long_runs_and_file_ends, "blocks": _c_blocks, "full_scale": _c_full_scale}
WORD_RUN_LAYOUTS = [n for n in LAYOUTS if n != "blocks"]


@functools.lru_cache(maxsize=None)
def _case(name, mode):
    """(pairs, ends, stop) - the same bursts for the walk and the kernels.  For the block mode the invalid words of the layouts lose their block flag as well,
    so the layout means the same there (`blocks` has block flags of its own, some against the word flags)."""
    pairs, bursts = LAYOUTS[name]()
    pairs = pairs.copy()
    if mode == CUBIC_BLOCK and name != "blocks":
        f = pairs["sample_flags"]
        pairs["sample_flags"] = np.where((f & A.SF_WORD_VALID) == 0, f & (0xFF ^ A.SF_BLOCK_OK), f).astype(np.uint8)
    n = len(pairs)
    ends = np.array([n] if bursts is None else sorted(set(min(n, max(1, int(round(x * n)))) for x in bursts) | {n}), dtype=np.uint64)
    return pairs, ends, 1


@functools.lru_cache(maxsize=None)
def _expected(name, mode):
    pairs, ends, stop = _case(name, mode)
    return W.run(pairs, mode, ends, stop)


def _sites(w, pairs_from, ln, ch):
    """the walk's cubic samples among the stream positions pairs_from + 1 .. + ln of channel ch (data pair d of a layout is stream position d + 1)"""
    return [s for s in w.cubic_sites if pairs_from + 1 <= s[0] <= pairs_from + ln and s[1] == ch]


def test_walk_windows_follow_the_closed_form():
    for name in ("singles_noise", "runs_1_to_8", "behind_the_kept_pairs", "above_is_last_entry"):
        pairs, ends, stop = _case(name, CUBIC_WORD)
        w = _expected(name, CUBIC_WORD)[3]
        n_stream = len(pairs) - 1           # the silent pair and the data pairs: the END_FILE tag is no entry
        assert [x[0] for x in w.windows] == [STRIDE * k for k in range(len(w.windows))] and len(w.windows) == -(-(n_stream - W.KEEP) // STRIDE), name
        assert all(x[1] == W.WIN for x in w.windows[:-1]) and w.windows[-1][1] == n_stream - STRIDE * (len(w.windows) - 1) and w.windows[-1][2], name


def test_the_layouts_are_what_they_are_meant_to_be():
    """What the walk says about every layout: which runs are cubic and which fall back."""
    ex = lambda name: _expected(name, CUBIC_WORD)
    w = ex("singles_noise")[3]
    assert len(w.cubic_sites) == 7 and len(ex("singles_tone")[3].cubic_sites) == 8      # (2222 / 2224 of the left channel: V I V I V)
    w = ex("runs_1_to_8")[3]
    for ln in range(1, 9):
        for s0, chs in ((200 + 100 * ln, (ln % 2,)), (1500 + 100 * ln, (0, 1))):
            for ch in chs:
                got = _sites(w, s0, ln, ch)
                assert len(got) == (ln if ln <= abi.AP_CUBIC_MAX_RUN else 0) and all(s[2] == ln + 1 for s in got), (ln, s0, ch)
    w = ex("v_i_v_i_v")[3]
    assert [s[0] for s in w.cubic_sites] == [901]                   # the outer neighbour is invalid: every other run is linear
    w = ex("outer_filled_earlier")[3]
    assert [s[0] for s in w.cubic_sites] == [at(2, 40) + 1]          # 509: its upper outer neighbour is invalid; 511: its lower one is masked by then
    assert (at(1, 511) + 1, 0, 2, True) in w.region_sites and ex("outer_filled_earlier")[0]["sample_flags"][at(1, 509) + 1, 0] & A.SF_WORD_MASKED
    w = ex("above_is_last_entry")[3]
    assert [s[0] for s in w.cubic_sites] == [at(4, 509) + 1]
    w = ex("behind_the_kept_pairs")[3]
    assert sorted(s[:2] for s in w.cubic_sites) == sorted([(2, 1)] + [(at(4, 3) + 1 + i, ch) for i in (0, 1) for ch in (0, 1)] + [(at(5, 3) + 1 + i, 1) for i in range(6)])
    out, _, _, w = ex("overlap_chain")
    _, runs = _overlap_chain_raw()
    second = {s + 1 for s, _, _ in runs[2::3]}
    assert {s[0] for s in w.cubic_sites} == second and len(second) == N_CHAINS >= 64
    for s, _, ch in runs[1::3]:          # entry 510 of every first window: filled with the word it held
        assert out["sample_flags"][s + 1, ch] & (A.SF_WORD_VALID | A.SF_WORD_MASKED) == A.SF_WORD_VALID
    assert len(ex("long_runs_and_file_ends")[3].cubic_sites) == 0
    assert len(_expected("blocks", CUBIC_BLOCK)[3].cubic_sites) > 20 and len(ex("blocks")[3].cubic_sites) > 20
    out, _, _, w = ex("full_scale")
    assert sorted(s[0] for s in w.cubic_sites) == [301, 301, 501, 501, 701, 701, 901, 901]
    assert [int(out["audio_word"][g, ch]) for g in (301, 501, 701, 901) for ch in range(2)] == [32767, 32767, 1, 1, -32768, -32768, 0, 0]


# ---- parity: the kernels against the walk ----------------------------------------------------------------------------------------------------------------
PARITY = [(n, m) for n in LAYOUTS for m in (CUBIC_BLOCK, CUBIC_WORD)]


def _parity(lib, via, oracle_lib, name, mode):
    pairs, ends, stop = _case(name, mode)
    want, want_pur, want_masked, w = _expected(name, mode)
    out, pur, masked = via.run(lib, pairs, mode, ends, stop)
    assert out.tobytes() == want.tobytes(), _diff(out, want)
    assert pur.tobytes() == want_pur.tobytes() and masked == want_masked
    # where nothing is cubic the output is the linear mode's (runs of 7 and 8, ramps, `altered` regions, file ends): against the oracle itself
    lin, _, lin_pur, lin_masked, _ = A.run_cpu(oracle_lib, "orc_", pairs, LIN_OF[mode], ends, stop)
    assert len(lin) == len(out) and lin_pur.tobytes() == pur.tobytes()
    cubic = np.zeros((len(out), 2), dtype=bool)
    pos = {int(g): i for i, g in enumerate(w.out_gids) if g >= 0}
    for g, ch, _ in w.cubic_sites:
        cubic[pos[g], ch] = True
    same = (out["audio_word"] == lin["audio_word"]) & (out["sample_flags"] == lin["sample_flags"])
    assert same[~cubic].all() and (len(w.cubic_sites) > 0 or (out.tobytes() == lin.tobytes() and masked == lin_masked)), name


@pytest.mark.parametrize("name,mode", PARITY)
def test_emu_parity(name, mode, emu_lib, oracle_lib):
    _parity(dc.emu_lib_of(emu_lib), dc.HOST, oracle_lib, name, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("name,mode", PARITY)
def test_gpu_parity(name, mode, oracle_lib):
    _parity(dc.product_lib(), dc.DEVICE, oracle_lib, name, mode)


def _in_place_and_staged_paths_agree(lib, via):
    """With room for the whole burst the pairs are worked on in place in the caller's buffer; with exactly the room the output needs they go through a buffer
    of the engine; with out_pairs == pairs the burst is copied first.  The walk's bytes on all three ways."""
    for name, mode in (("runs_1_to_8", CUBIC_WORD), ("singles_tone", CUBIC_WORD), ("overlap_chain", CUBIC_WORD), ("blocks", CUBIC_BLOCK)):
        pairs, ends, stop = _case(name, mode)
        want, want_pur, want_masked, _ = _expected(name, mode)
        eng = lib.sdv_engine_create(0)
        assert lib.sdv_set_audio_masking(eng, mode) == 0
        outs, a, total = [], 0, 0
        for k, b in enumerate(ends):
            b = int(b)
            st = 1 if (stop and k + 1 == len(ends)) else 0
            rc, o, _, _, n_out, n_pur = via.audio(lib, eng, pairs[a:b], st, out_cap=0)          # refused: tells the size, takes nothing
            if rc == 0:
                assert n_out == 0
            else:
                assert rc == -1 and n_out > 0
                rc, o, p, m, n_out2, _ = via.audio(lib, eng, pairs[a:b], st, out_cap=n_out, purges_cap=max(n_pur, 1))
                assert rc == 0 and n_out2 == n_out
                total += m
            outs.append(o.copy()); a = b
        out = np.concatenate(outs)
        assert out.tobytes() == want.tobytes() and total == want_masked, name + ": " + _diff(out, want)
        # out_pairs == pairs
        assert lib.sdv_reset_audio(eng) == 0
        buf = via.array(np.concatenate([pairs, np.zeros(1024, dtype=PAIR_DTYPE)]))
        pur = via.zeros(16, A.PURGE_DTYPE)
        n_out, n_pur, nm = C.c_size_t(0), C.c_size_t(0), C.c_uint64(0)
        ptr = via.ptr(buf)
        rc = lib.sdv_audio_process(eng, ptr, len(pairs), 1, ptr, len(buf), C.byref(n_out), via.ptr(pur), 16, C.byref(n_pur), C.byref(nm), via.stream())
        lib.sdv_engine_destroy(eng)
        via.check(pur)
        if len(ends) == 1:
            assert rc == 0 and via.get(buf, n_out.value).tobytes() == want.tobytes() and nm.value == want_masked, name


def test_emu_in_place_and_staged_paths_agree(emu_lib):
    _in_place_and_staged_paths_agree(dc.emu_lib_of(emu_lib), dc.HOST)


@pytest.mark.gpu
def test_gpu_in_place_and_staged_paths_agree():
    _in_place_and_staged_paths_agree(dc.product_lib(), dc.DEVICE)


# ---- untouched behaviour, refusals ---------------------------------------------------------------------------------------------------------------------------
def _run_on(lib, via, eng, pairs, ends, stop):
    """the bursts of a case on an engine that lives on: from a reset stream, in the mode it has -> (out, purges, masked)"""
    assert lib.sdv_reset_audio(eng) == 0
    outs, purs, masked, a, got = [], [], 0, 0, 0
    for k, b in enumerate(ends):
        b = int(b)
        rc, o, p, m, _, _ = via.audio(lib, eng, pairs[a:b], 1 if (stop and k + 1 == len(ends)) else 0)
        assert rc == 0, lib.sdv_last_error(eng)
        p = p.copy()
        p["first_pair"] += got
        p["tag_index"] += a
        outs.append(o.copy()); purs.append(p); masked += m
        got += len(o); a = b
    return np.concatenate(outs), np.concatenate(purs), masked


def _old_modes_are_untouched(lib, via, oracle_lib):
    """Modes 0..6 on one engine, a cubic call, modes 0..6 again: the same bytes, which are the oracle's.  The mode is the only state the setter touches."""
    eng = lib.sdv_engine_create(0)
    for name in ("short_runs_lin", "window_edges", "bursts_long_runs"):
        pairs, _, ends, stop = A.make_input(name)
        rounds = []
        for _ in range(2):
            got = []
            for mode in range(7):
                assert lib.sdv_set_audio_masking(eng, mode) == 0
                got.append(_run_on(lib, via, eng, pairs, ends, stop))
            rounds.append(got)
            assert lib.sdv_set_audio_masking(eng, CUBIC_WORD) == 0
            c = _run_on(lib, via, eng, pairs, ends, stop)
            want = W.run(pairs, CUBIC_WORD, ends, stop)
            assert c[0].tobytes() == want[0].tobytes() and c[1].tobytes() == want[1].tobytes() and c[2] == want[2]
        for mode in range(7):
            o, _, p, m, _ = A.run_cpu(oracle_lib, "orc_", pairs, mode, ends, stop)
            for got in rounds:
                assert got[mode][0].tobytes() == o.tobytes() and got[mode][1].tobytes() == p.tobytes() and got[mode][2] == m, (name, mode)
    lib.sdv_engine_destroy(eng)


def test_emu_old_modes_are_untouched(emu_lib, oracle_lib):
    _old_modes_are_untouched(dc.emu_lib_of(emu_lib), dc.HOST, oracle_lib)


@pytest.mark.gpu
def test_gpu_old_modes_are_untouched(oracle_lib):
    _old_modes_are_untouched(dc.product_lib(), dc.DEVICE, oracle_lib)


def _refusals(lib, via, oracle_lib):
    """8 and 9 are modes; 7 (SDV_DROP_MAX), -1, 10 and 255 are refused and leave the mode as it was - seen by what the next call does."""
    pairs, ends, stop = _case("runs_1_to_8", CUBIC_WORD)
    eng = lib.sdv_engine_create(0)
    for good in (CUBIC_BLOCK, CUBIC_WORD, A.DROP_HOLD_WORD, CUBIC_WORD):
        assert lib.sdv_set_audio_masking(eng, good) == abi.OK
        for bad in (7, -1, 10, 255):
            assert lib.sdv_set_audio_masking(eng, bad) == abi.ERR_BAD_ARG and b"no such masking mode" in lib.sdv_last_error(eng)
        out, pur, masked = _run_on(lib, via, eng, pairs, ends, stop)
        if good == A.DROP_HOLD_WORD:
            want, _, want_pur, want_masked, _ = A.run_cpu(oracle_lib, "orc_", pairs, good, ends, stop)
        else:
            want, want_pur, want_masked, _ = W.run(pairs, good, ends, stop)
        assert out.tobytes() == want.tobytes() and pur.tobytes() == want_pur.tobytes() and masked == want_masked, good
    lib.sdv_engine_destroy(eng)
    assert lib.sdv_set_audio_masking(None, CUBIC_WORD) == abi.ERR_BAD_ARG
    assert (abi.DROP_INTER_CUBIC_BLOCK, abi.DROP_INTER_CUBIC_WORD, abi.AP_CUBIC_MAX_RUN, abi.DROP_MAX) == (8, 9, 6, 7) and lib.sdv_abi_version() >= 14


def test_emu_refusals(emu_lib, oracle_lib):
    _refusals(dc.emu_lib_of(emu_lib), dc.HOST, oracle_lib)


@pytest.mark.gpu
def test_gpu_refusals(oracle_lib):
    _refusals(dc.product_lib(), dc.DEVICE, oracle_lib)


# ---- purpose ---------------------------------------------------------------------------------------------------------------------------------------------------
AMP, FS, EVERY, N_SITES, PEAK_SITE = 10000.0, 44056.0, 64, 60, 5


@functools.lru_cache(maxsize=None)
def _tone_tape(hz):
    """Both channels carry the tone A sin(w t + phase), rounded to int16; one invalid word every 64 pairs, the channels taking turns, the word itself garbage.
    The phase puts site PEAK_SITE on a crest, where a straight line is at its worst.  Sites the walk calls a fallback are left undamaged.
    -> (pairs, the unrounded tone per data pair, [(data pair, channel)], w)"""
    w = 2 * math.pi * hz / FS
    n = EVERY * (N_SITES + 1)
    first = 40
    tone = AMP * np.sin(w * np.arange(n) + (math.pi / 2 - w * (first + EVERY * PEAK_SITE)))
    sites = [(first + EVERY * j, j % 2) for j in range(N_SITES)]
    rng = np.random.default_rng(11)
    garbage = rng.integers(-32768, 32768, N_SITES)

    def build(which):
        a = np.zeros(n, dtype=PAIR_DTYPE)
        a["audio_word"] = np.rint(tone)[:, None]
        a["sample_flags"] = A.SF_BLOCK_OK | A.SF_WORD_VALID
        a["sample_rate"] = 44056
        for j, (d, ch) in enumerate(sites):
            if (d, ch) in which:
                a["audio_word"][d, ch] = garbage[j]
                a["sample_flags"][d, ch] = A.SF_BLOCK_OK
        return A.tape(["N", a, "E"])

    cubic = {(g - 1, ch) for g, ch, _ in W.run(build(set(sites)), CUBIC_WORD, [n + 2], 1)[3].cubic_sites}
    kept = [s for s in sites if s in cubic]
    pairs = build(set(kept))
    assert {(g - 1, ch) for g, ch, _ in W.run(pairs, CUBIC_WORD, [n + 2], 1)[3].cubic_sites} == set(kept) and sites[PEAK_SITE] in kept and len(kept) >= N_SITES - 4
    return pairs, tone, kept, w


def _purpose(lib, via, hz):
    """At the invalid words mode 9 errs against the unrounded tone by at most A |1 - (4 cos w - cos 2w) / 3| (the interpolant (-1, 4, 4, -1) / 6 on a sine)
    + 0.5 (the output's rounding) + 0.5 * 10 / 6 (the four inputs' roundings through the weights, whose magnitudes sum to 10 / 6); mode 6 on the same tape
    errs by at least A (1 - cos w) - 1 at the site on the crest: the mean of two neighbours of a crest is A cos w, their two roundings move it by at most
    0.5 and the rounding of the line's own arithmetic by at most 0.5.  About 2 and 100 LSB at 997 Hz."""
    pairs, tone, sites, w = _tone_tape(hz)
    ends = np.array([len(pairs)], dtype=np.uint64)
    bound_cubic = AMP * abs(1 - (4 * math.cos(w) - math.cos(2 * w)) / 3) + 0.5 + 0.5 * 10 / 6
    bound_lin = AMP * (1 - math.cos(w)) - 1
    err = {}
    for mode in (CUBIC_WORD, A.DROP_INTER_LIN_WORD):
        out, _, masked = via.run(lib, pairs, mode, ends, 1)
        assert len(out) == len(tone) and masked <= len(sites)          # the silent pair in front, the last data pair dropped by the purge: out[d + 1] is data pair d
        err[mode] = np.array([abs(float(out["audio_word"][d + 1, ch]) - tone[d]) for d, ch in sites])
        untouched = np.ones((len(tone) - 1, 2), dtype=bool)
        for d, ch in sites:
            untouched[d, ch] = False
        assert (out["audio_word"][1:][untouched] == np.rint(tone)[:-1, None].repeat(2, axis=1)[untouched]).all()
    print("%g Hz: mode 9 max error %.3f (bound %.3f), mode 6 max error %.3f (at least %.3f)" % (hz, err[CUBIC_WORD].max(), bound_cubic, err[A.DROP_INTER_LIN_WORD].max(), bound_lin))
    assert err[CUBIC_WORD].max() <= bound_cubic
    assert err[A.DROP_INTER_LIN_WORD].max() >= bound_lin
    assert bound_cubic < bound_lin


@pytest.mark.parametrize("hz", [997.0, 5000.0])
def test_emu_purpose(hz, emu_lib):
    _purpose(dc.emu_lib_of(emu_lib), dc.HOST, hz)


@pytest.mark.gpu
@pytest.mark.parametrize("hz", [997.0, 5000.0])
def test_gpu_purpose(hz):
    _purpose(dc.product_lib(), dc.DEVICE, hz)


# ---- the fused entry, the C++ example -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _damaged_tape():
    """tests/tape_truth.py: a 14-bit sine tape of four frames with 48 lines of one field black - blocks beyond the code's reach, runs of one and two invalid samples"""
    import encode_api as en
    import tape_truth as tt
    d = tt.geometry(en.NTSC, en.BIT14)
    pcm, w9, luma = tt.make_tape(en.NTSC, en.BIT14, 4, "sine", d=d)
    return tt.apply(luma, tt.burst_at_row(w9, d, 1, 200, 48), d)


def _fused_equals_separate_calls(lib, via):
    """sdv_decode_frames with with_audio = 1 in mode 9 == its pair stream without the audio stage through sdv_audio_process in mode 9 == the walk on that stream."""
    import tape_truth as tt
    luma = _damaged_tape()
    raw, frames, _ = tt.decode(via, lib, luma)
    got, got_frames, masked = tt.decode(via, lib, luma, mask_mode=CUBIC_WORD)
    ends = np.array([len(raw)], dtype=np.uint64)
    want, _, want_masked = via.run(lib, raw, CUBIC_WORD, ends, 1)
    assert got.tobytes() == want.tobytes() and masked == want_masked and got_frames.tobytes() == frames.tobytes()
    walk, _, walk_masked, w = W.run(raw, CUBIC_WORD, ends, 1)
    assert got.tobytes() == walk.tobytes() and masked == walk_masked and len(w.cubic_sites) > 100


def test_emu_fused_equals_separate_calls(emu_lib):
    _fused_equals_separate_calls(dc.emu_lib_of(emu_lib), dc.HOST)


@pytest.mark.gpu
def test_gpu_fused_equals_separate_calls():
    _fused_equals_separate_calls(dc.product_lib(), dc.DEVICE)


@pytest.mark.gpu
def test_gpu_cpp_example_writes_the_cubic_wav(tmp_path):
    """decode_tape wav ... 9 from plain C++ == the bytes Engine gives for the same file (binarize -> stitch -> audio_process in mode 9 -> wav_files); and not
    the file of mode 6: the argument reaches the setter."""
    import subprocess
    import torch
    from sdvpcmdecoder_amd import Engine, build as b
    import stitch_api as sa
    import test_stitch_kernel as tsk
    exe = b.build_example()
    luma = _damaged_tape()
    n, h, wd = luma.shape
    (tmp_path / "luma.raw").write_bytes(np.ascontiguousarray(luma).tobytes())
    files = {}
    for mode in (CUBIC_WORD, A.DROP_INTER_LIN_WORD):
        name = tmp_path / ("out%d.wav" % mode)
        out = subprocess.run([exe, "wav", str(tmp_path / "luma.raw"), str(wd), str(h), str(n), str(name), str(mode)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr + out.stdout
        files[mode] = name.read_bytes()
    eng = Engine(0)
    lines, _ = eng.binarize_frames(torch.from_numpy(luma).cuda(), first_frame_no=1, new_file=True, end_file=True)
    eng.set_stitch_settings(tsk._settings(sa.default_settings()))
    pairs, _ = eng.stitch_frames(lines)
    eng.set_audio_masking(CUBIC_WORD)
    out, pur, masked = eng.audio_process(pairs, stop=True)
    assert masked > 0 and eng.wav_files(out, pur) == {0: files[CUBIC_WORD]}
    assert files[CUBIC_WORD] != files[A.DROP_INTER_LIN_WORD] and len(files[CUBIC_WORD]) == len(files[A.DROP_INTER_LIN_WORD])
