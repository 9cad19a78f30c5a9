"""Tapes that steer sdv_binarize_frames onto each build of the STC-007 frame kernel (stc007_frames_engine.inc: run_round_range / run_round_lists, prepare_memo,
settle_sweeps), as streams of
several calls.  Shared by the emulator tests, the GPU tests against the oracle (test_gpu_kernel_paths.py) and the child process that runs them through the
developer build of the HIP library, counts the launches and decodes every tape again under each off-switch of the scheduler."""
import numpy as np

from sdvpcmdecoder_amd import synth

# the scheduler's off-switches (read by developer builds only: engine.inc dev_env; stc007_frames_engine.inc reads them)
SWITCHES = ("SDV_NO_FAT", "SDV_NO_TC", "SDV_SCHED_NO_SIG", "SDV_SCHED_NO_PASS", "SDV_SCHED_NO_SKIP", "SDV_SCHED_NO_CARRY", "SDV_NO_PREDICT_IN_KERNEL")


def unreadable_cells(luma, every=53, seed=53):
    """A bit cell inverted on one line in `every` (test_gpu_parity._unreadable_cells): no reference level reads such a line, MODE_NORMAL sweeps every level."""
    rng = np.random.default_rng(seed)
    out = luma.copy()
    flat = out.reshape(-1, out.shape[-1])
    w = flat.shape[1]
    for r in range(0, flat.shape[0], every):
        x = 12 + int(rng.integers(4, 132)) * (w - 24) // 137
        flat[r, x:x + 5] = np.clip(230 - flat[r, x:x + 5].astype(np.int16), 0, 255).astype(np.uint8)
    return out


def worn_tape(n_frames, height, seed=31):
    """An unreadable cell in every fifth line (test_emu_worn_tape_without_meetings_...): every frame goes through the general kernel and hardly a decode meets
    the frame's last pass - the engine gives the calls behind the first to the build without snapshots, and every eighth of them back to the snapshots."""
    luma0, _, _ = synth.stc007_frames(n_frames, seed=seed, height=height, noise_sigma=4.0)
    lum = luma0.copy()
    flat = lum.reshape(-1, 720)
    rng = np.random.default_rng(5)
    rows = np.arange(3, flat.shape[0], 5)
    xs = 12 + (rng.integers(4, 132, size=rows.shape) * (720 - 24)) // 137
    for dx in range(5):
        flat[rows, xs + dx] = np.clip(230 - flat[rows, xs + dx].astype(np.int16), 0, 255).astype(np.uint8)
    return lum


def _shifted(luma0, jumps):
    luma = luma0.copy()
    for f, to in jumps:
        luma[f:] = np.roll(luma0[f:], to, axis=2)
    return luma


def _pass_meets_tape(n, height, seed):
    luma0, _, _ = synth.stc007_frames(n, seed=seed, height=height, noise_sigma=4.0)
    lum = luma0.copy()
    lum[:, 16::17, :] = 16
    flat = lum.reshape(-1, 720)
    rng = np.random.default_rng(53)
    rows = np.arange(0, flat.shape[0], 11)
    xs = 12 + (rng.integers(4, 132, size=rows.shape) * (720 - 24)) // 137
    for dx in range(5):
        flat[rows, xs + dx] = np.clip(230 - flat[rows, xs + dx].astype(np.int16), 0, 255).astype(np.uint8)
    return np.concatenate([luma0[:8], lum]), [8, n]


def _mark_tape():
    clean, _, _ = synth.stc007_frames(30, seed=91, noise_sigma=3.0, height=96, lines_per_field=48)
    worn = unreadable_cells(clean[13:25].copy(), every=7)
    more, _, _ = synth.stc007_frames(40, seed=92, noise_sigma=3.0, height=96, lines_per_field=48)
    return np.concatenate([clean[:13], worn, more[:24]]), [1, 12, 12, 12, 12]


def _general_shift_tape():
    luma, _, _ = synth.stc007_frames(8, seed=612, height=240, noise_sigma=4.0)
    luma = luma.copy()
    luma[2:] = np.roll(luma[2:], -2, axis=2)
    luma[4, 3] = 16; luma[6, 8] = 16; luma[6, 150] = 16
    return luma, [8]


def _crowd_waits_tape():
    luma, _, _ = synth.stc007_frames(40, seed=77, noise_sigma=4.0)
    return np.ascontiguousarray(unreadable_cells(luma)[:12]), [12]


def _crowd_windows_tape():
    luma0, _, _ = synth.stc007_frames(160, seed=5, height=24, noise_sigma=3.0)
    return np.concatenate([luma0[:20], _shifted(luma0, [(30, 6), (55, -7), (80, 4), (105, -5), (130, 8)])]), [20, 160]


def _model_skip_tape():
    luma0, _, _ = synth.stc007_frames(120, seed=9, height=24, noise_sigma=3.0)
    return np.concatenate([luma0[:20], _shifted(luma0, [(25, 6), (50, -7), (90, 5)])]), [20, 120]


def _big_round_tape():
    luma, _, _ = synth.stc007_frames(1200, seed=83, height=96, lines_per_field=48, noise_sigma=4.0)
    return np.ascontiguousarray(unreadable_cells(luma, every=23)), [600, 600]


# name -> () -> (luma of the whole stream (n, height, 720), frames per call); every stream is decoded in MODE_NORMAL from a new file
TAPES = {
    "worn_plain_reprobe": lambda: (worn_tape(120, 96), [12] * 10),
    "worn_mark_comes_and_goes": _mark_tape,
    "big_round_with_sweeps": _big_round_tape,
    "crowd_over_several_windows": _crowd_windows_tape,
    "pass_meets_last_30x64": lambda: _pass_meets_tape(30, 64, 3),
    "pass_meets_last_16x200": lambda: _pass_meets_tape(16, 200, 9),
    "cold_chain_first_sweep": lambda: (synth.stc007_frames(4, seed=14, height=64, noise_sigma=3.0)[0], [4]),
    "crowd_waits_for_first_frame": _crowd_waits_tape,
    "general_kernel_later_shift_stage": _general_shift_tape,
    "model_gives_old_state": _model_skip_tape,
}


# What every call of a stream costs, (rounds, frames_launched, frames_general, sweeps, frames_met) of sdv_run_info: records that equal the sequential oracle's
# say that the schedule settled, not which schedule it was - any that settles gives them.  The emulator's figures are deterministic; taken before the frame
# entry was split into a plan and a driver (profiles/stc007_scheduler_notes.md), they pin the scheduler's decisions round by round.
# (big_round_with_sweeps, worn_plain_reprobe and pass_meets_last_16x200 are not decoded on the emulator at these sizes: GPU_SCHEDULE has them.)
SCHEDULE = {
    "cold_chain_first_sweep": [(2, 4, 1, 1, 0)],
    "general_kernel_later_shift_stage": [(4, 13, 4, 1, 0)],
    "crowd_waits_for_first_frame": [(6, 42, 21, 103, 0)],
    "crowd_over_several_windows": [(2, 20, 1, 1, 0), (7, 516, 113, 0, 37)],
    "model_gives_old_state": [(2, 20, 1, 1, 0), (7, 362, 65, 0, 23)],
    "pass_meets_last_30x64": [(2, 8, 1, 1, 0), (7, 119, 64, 156, 0)],
    "worn_mark_comes_and_goes": [(1, 1, 1, 1, 0), (1, 12, 0, 0, 0), (7, 47, 24, 153, 0), (1, 12, 12, 0, 0), (1, 12, 0, 0, 0)],
}
# ... and crowd_over_several_windows under each off-switch: every switch goes on steering the code it steered
SWITCH_SCHEDULE = {
    "SDV_NO_FAT": [(3, 21, 2, 1, 0), (7, 516, 113, 0, 37)],
    "SDV_NO_TC": [(2, 20, 1, 1, 0), (7, 516, 113, 0, 0)],
    "SDV_SCHED_NO_SIG": [(2, 20, 1, 1, 0), (9, 702, 341, 0, 45)],
    "SDV_SCHED_NO_PASS": SCHEDULE["crowd_over_several_windows"],
    "SDV_SCHED_NO_SKIP": SCHEDULE["crowd_over_several_windows"],
    "SDV_SCHED_NO_CARRY": [(2, 20, 1, 1, 0), (13, 560, 116, 0, 37)],
    "SDV_NO_PREDICT_IN_KERNEL": SCHEDULE["crowd_over_several_windows"],
}

# The same on the MI355X (test_gpu_kernel_paths.test_gpu_tape_equals_the_sequential_oracle): every tape decoded twice there gave the same figures both times,
# and the emulator's where the emulator decodes the tape - so the GPU column is the emulator's, with the three tapes only the GPU decodes at this size.
GPU_SCHEDULE = dict(SCHEDULE)
GPU_SCHEDULE.update({
    "worn_plain_reprobe": [(7, 44, 23, 211, 0), (3, 35, 35, 217, 0), (4, 36, 36, 215, 0), (3, 34, 34, 212, 0), (3, 35, 35, 218, 0), (5, 47, 47, 223, 0), (3, 35, 35, 215, 0),
                           (5, 40, 40, 210, 0), (5, 42, 42, 216, 0), (3, 35, 35, 214, 0)],
    "big_round_with_sweeps": [(13, 4204, 3007, 2771, 7), (14, 3366, 3366, 2518, 0)],
    "pass_meets_last_16x200": [(2, 8, 1, 1, 0), (7, 63, 34, 262, 0)],
})


def schedule_of(info):
    return (info.rounds, info.frames_launched, info.frames_general, info.sweeps, info.frames_met)


def run_stream(call, luma, calls):
    """Decodes luma in calls of the given sizes through call(chunk, first_frame_no, new_file) -> (recs, stats, info, extra); returns the records and frame
    stats of the whole stream and the (info, extra) of every call."""
    recs, stats, per_call = [], [], []
    k = 0
    for cnt in calls:
        r, s, info, extra = call(np.ascontiguousarray(luma[k:k + cnt]), 1 + k, k == 0)
        recs.append(np.asarray(r).view(np.uint8).reshape(-1)); stats.append(np.asarray(s).view(np.uint8).reshape(-1))
        per_call.append((info, extra))
        k += cnt
    assert k == len(luma)
    return np.concatenate(recs), np.concatenate(stats), per_call


def check_counts(name, counts, switch=None):
    """What the launch counts of each call (engine_api.launch_counts) have to show for the tape: the build it was made for ran.  Returns None or a message."""
    gen = lambda c: c["snap_frames"] + c["plain_frames"] + c["fat_frames"]
    if switch == "SDV_NO_FAT" and any(c["fat"] for c in counts):
        return "the five-wave kernel ran under SDV_NO_FAT"
    if switch == "SDV_NO_TC" and any(c["snap"] for c in counts):
        return "the snapshot build ran under SDV_NO_TC"
    if switch is not None:
        return None
    if name == "worn_plain_reprobe":
        # call 1 (snapshots armed) decides on the plain build: calls 2-8 take it, call 9 looks again with the snapshots, call 10 is plain again
        for i, c in enumerate(counts):
            if i in (1, 2, 3, 4, 5, 6, 7, 9) and not (c["plain_frames"] >= 12 and c["snap"] == 0):
                return "call %d: the plain build was meant to run" % (i + 1)
            if i == 8 and not (c["snap_frames"] >= 12 and c["plain"] == 0):
                return "call 9: the snapshot build was meant to run (the re-probe)"
            if i == 0 and c["plain"] != 0:
                return "call 1: the plain build ran before the engine had looked at the tape"
    elif name == "worn_mark_comes_and_goes":
        if not (counts[0]["fat_frames"] == 1 and counts[0]["lean"] == 0):
            return "the cold frame alone: the five-wave kernel"
        if not (counts[1]["lean_frames"] >= 12 and gen(counts[1]) == 0):
            return "a clean call behind the cold frame: the lean kernel only"
        if not gen(counts[2]) > 0:
            return "the damaged call: frames through the general kernel"
        if not (counts[3]["snap_frames"] + counts[3]["plain_frames"] >= 12):
            return "the call behind the worn one starts every frame on the general kernel"
        if not (counts[4]["lean_frames"] >= 12 and gen(counts[4]) == 0):
            return "the mark came off: the lean kernel again"
    elif name == "big_round_with_sweeps":
        c = counts[1]
        # the worn call's first round sends all 600 frames to a general build that does not settle sweeps; they are settled by sdv_k_stc007_sweep_levels / _pick
        if not (c["snap_frames"] + c["plain_frames"] >= 600 and (c["snap"] + c["plain"]) >= 1 and c["sweep_levels_reqs"] > 0 and c["sweep_pick_reqs"] == c["sweep_levels_reqs"]):
            return "the round of 600 general frames with its sweeps settled off the frame kernel"
        if not counts[0]["fat_frames"] >= 1:
            return "the cold first frame: the five-wave kernel"
    elif name == "cold_chain_first_sweep":
        if not (counts[0]["fat"] == 1 and counts[0]["fat_frames"] == 1):
            return "the cold first frame: the five-wave kernel, once"
    return None
