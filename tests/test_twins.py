"""Every emulator test has a GPU test beside it.  The SIMT emulator runs one wave at a time on host memory and ignores the stream:
it cannot see a race between waves, a read-after-write between workgroups of a call in place, work on the wrong stream, a launch at an estimated width,
LDS limits or code generation.  So for every `test_emu_<x>` of tests/test_*.py one of these holds:

  (a) the same module has a `test_gpu_<x>` with the `gpu` mark that calls the same body function (written once for both, handed
      device_calls.HOST or .DEVICE, a back end or a library);
  (b) COVERED_BY names the GPU test that covers it, as "module::name" - that test exists and carries the `gpu` mark;
  (c) COVERED_BY says "emulator only: <reason>".

NOT_YET_TWINNED was the open rest, from tests/test_emu_parity.py (the STC-007 front half): it is empty and stays empty - a new emulator test comes with
its twin, or with its reason."""
import ast
import glob
import os

HERE = os.path.dirname(os.path.abspath(__file__))

_KP = "test_gpu_kernel_paths::test_gpu_tape_equals_the_sequential_oracle"      # (one case per tape of tests/kernel_path_tapes.py)
COVERED_BY = {
    # ---- the STC-007 front half: tests/test_emu_parity.py against test_gpu_parity.py (test_hip_*) and test_gpu_kernel_paths.py, read side by side
    "test_emu_parity::test_emu_small_frames": "test_gpu_parity::test_hip_vs_oracle_degraded",                       # the four modes against the oracle
    "test_emu_parity::test_emu_end_of_file_frame_and_next_source": "test_gpu_parity::test_gpu_end_of_file_frame_and_next_source",      # the same tapes
    "test_emu_parity::test_emu_batch_path_corner_cases": "test_gpu_parity::test_gpu_batch_path_corner_cases",                          # the same tapes
    "test_emu_parity::test_emu_ragged_geometry": "test_gpu_parity::test_hip_ragged_geometry",
    "test_emu_parity::test_emu_golden_rough_draft": "test_gpu_parity::test_hip_matches_reference_golden",          # every case of golden_cases.CASES
    "test_emu_parity::test_emu_speculation_rounds": "test_gpu_parity::test_hip_stream_continuation_and_rounds",
    "test_emu_parity::test_emu_misprediction_is_repaired": "test_gpu_parity::test_hip_window_jumps_far_and_near",
    "test_emu_parity::test_emu_random_dropouts_and_anchors": "test_gpu_parity::test_hip_dropouts_across_calls",
    "test_emu_parity::test_emu_window_jump_settles_in_few_rounds": _KP,                                             # crowd_over_several_windows: rounds <= 8
    "test_emu_parity::test_emu_crowd_over_several_windows_is_led_by_the_first_frame_of_each": _KP,                 # crowd_over_several_windows
    "test_emu_parity::test_emu_a_pass_that_meets_the_last_one_changes_nothing": _KP,                               # pass_meets_last_30x64 / _16x200
    "test_emu_parity::test_emu_cold_chain_settles_its_first_sweep_in_one_pass": _KP,                               # cold_chain_first_sweep
    "test_emu_parity::test_emu_small_rounds_settle_their_sweeps_themselves": "test_gpu_parity::test_hip_small_rounds_settle_their_sweeps_themselves",
    "test_emu_parity::test_emu_tape_that_sits_on_a_later_shift_stage": "test_gpu_parity::test_hip_tape_that_sits_on_a_later_shift_stage",
    "test_emu_parity::test_emu_general_kernel_on_a_later_shift_stage": _KP,                                        # general_kernel_later_shift_stage
    "test_emu_parity::test_emu_frames_the_model_gives_their_old_state_are_not_decoded_again": _KP,                 # model_gives_old_state
    "test_emu_parity::test_emu_worn_tape_without_meetings_takes_the_plain_general_kernel": _KP,                    # worn_plain_reprobe
    "test_emu_parity::test_emu_bad_arguments": "test_gpu_kernel_paths::test_gpu_bad_arguments",
    "test_emu_parity::test_emu_tall_frames_keep_their_histories": "test_gpu_kernel_paths::test_gpu_tall_frames_keep_their_histories",
    "test_emu_parity::test_emu_worn_tape_mark_comes_and_goes": _KP,                                                # worn_mark_comes_and_goes
    "test_emu_parity::test_emu_unreadable_cells_sweep_every_level": "test_gpu_parity::test_hip_unreadable_cells_sweep_every_level",
    "test_emu_parity::test_emu_crowd_waits_for_the_sweeps_of_its_first_frame": _KP,                                # crowd_waits_for_first_frame
    "test_emu_parity::test_emu_lines_that_read_on_other_rungs_of_the_ladder": "test_gpu_parity::test_hip_lines_that_read_on_other_rungs_of_the_ladder",
    "test_emu_parity::test_emu_worn_tape_plain_build_and_its_reprobe": _KP,                                        # worn_plain_reprobe
    "test_emu_parity::test_emu_schedule_of_the_tape_whose_passes_meet": _KP,                                       # pass_meets_last_30x64
    "test_emu_parity::test_emu_every_switch_steers_what_it_steered": "test_gpu_kernel_paths::test_gpu_kernel_paths_on_a_developer_build",     # every tape under every switch
    # ---- pairs by name that are written separately (the GPU test goes through sdvpcmdecoder_amd.Engine, often on more or larger cases): named on purpose
    "test_audio::test_emu_matches_oracle": "test_audio::test_gpu_matches_oracle",
    "test_audio::test_emu_random_tapes": "test_audio::test_gpu_random_tapes",
    "test_decode_frames::test_emu_fused_equals_separate_calls": "test_decode_frames::test_gpu_fused_equals_separate_calls",
    "test_decode_frames::test_emu_fused_stream_in_calls_equals_one_call": "test_decode_frames::test_gpu_fused_stream_in_calls_equals_one_call",
    "test_decode_frames::test_emu_fused_uneven_calls_equal_the_sequential_oracle": "test_decode_frames::test_gpu_fused_uneven_calls_equal_the_sequential_oracle",
    "test_decode_frames::test_emu_fused_direct_frames_other_geometries": "test_decode_frames::test_gpu_fused_direct_frames_other_geometries",
    "test_decode_frames::test_emu_fused_stitch_queued_ahead_is_made_over_when_the_frame_stage_needs_more_rounds":
        "test_decode_frames::test_gpu_fused_stitch_queued_ahead_is_made_over_when_the_frame_stage_needs_more_rounds",
    "test_markerless_geometry::test_emu_frames_in_awkward_buffers": "test_markerless_geometry::test_gpu_frames_in_awkward_buffers",
    "test_markerless_geometry::test_emu_stream_in_awkward_buffers": "test_markerless_geometry::test_gpu_stream_in_awkward_buffers",
    "test_markerless_geometry::test_emu_lines_in_awkward_buffers": "test_markerless_geometry::test_gpu_lines_in_awkward_buffers",
    "test_markerless_geometry::test_emu_fused_call_in_an_awkward_buffer": "test_markerless_geometry::test_gpu_fused_call_in_an_awkward_buffer",
    "test_markerless_geometry::test_emu_refuses_geometry_it_cannot_take": "test_markerless_geometry::test_gpu_refuses_geometry_it_cannot_take",
    "test_pcm1::test_emu_matches_oracle": "test_pcm1::test_gpu_matches_oracle",
    "test_pcm16::test_emu_matches_oracle": "test_pcm16::test_gpu_matches_oracle",
    "test_pcm1_frames::test_emu_matches_oracle": "test_pcm1_frames::test_gpu_matches_oracle",
    "test_pcm16_frames::test_emu_matches_oracle": "test_pcm16_frames::test_gpu_matches_oracle",
    "test_pcm1_front::test_emu_matches_oracle": "test_pcm1_front::test_gpu_matches_oracle",
    "test_pcm16_front::test_emu_lines_match_oracle": "test_pcm16_front::test_gpu_lines_match_oracle",
    "test_pcm1_vis::test_emu_matches_oracle": "test_pcm1_vis::test_gpu_matches_oracle",
    "test_render::test_emu_matches_oracle": "test_render::test_gpu_matches_oracle",
    "test_render::test_emu_blocks_and_their_canvases_match_oracle": "test_render::test_gpu_blocks_and_their_canvases_match_oracle",
    "test_render::test_emu_asm_lines_and_their_canvases_match_oracle": "test_render::test_gpu_asm_lines_and_their_canvases_match_oracle",
    "test_stc_lines::test_emu_lines_equal_the_oracle": "test_stc_lines::test_gpu_lines_equal_the_oracle",
    "test_stc_lines::test_emu_lines_other_shapes": "test_stc_lines::test_gpu_lines_other_shapes",
    "test_stitch_kernel::test_emu_matches_oracle": "test_stitch_kernel::test_gpu_matches_oracle",
    # ---- covered by a GPU test of another name
    "test_decode_frames::test_emu_fused_direct_frames_decoded_again_with_records": "test_decode_frames::test_gpu_fused_way_back_with_records_on_a_developer_build",
    "test_deint_kernel::test_emu_deint_matches_oracle": "test_deint_kernel::test_hip_deint_matches_oracle",
    "test_dropped_frames::test_emu_matches_oracle": "test_dropped_frames::test_gpu_matches_golden_from_reference",      # the same cases, against the fixtures the oracle is pinned to
    "test_dropped_frames::test_emu_double_width_feeds_the_doubled_path": "test_dropped_frames::test_gpu_double_width",
    "test_pcm16::test_emu_long_tape_matches_oracle": "test_pcm16::test_gpu_long_damaged_tape_matches_oracle",
    "test_pcm16_asm::test_emu_lines_match_oracle": "test_pcm16_asm::test_gpu_lines_and_window_match_oracle",
    "test_pcm16_vis::test_emu_blocks_match_oracle": "test_pcm16_vis::test_gpu_blocks_and_canvases_match_oracle",
    "test_pcm1_frames::test_emu_stream_in_two_calls": "test_pcm1_frames::test_gpu_stream_in_pieces_equals_oracle",
    "test_pcm16_frames::test_emu_stream_in_two_calls": "test_pcm16_frames::test_gpu_stream_in_pieces_equals_oracle",
    "test_render::test_emu_pcm1_stitcher_canvases_match_oracle": "test_render::test_gpu_pcm1_stitcher_feeds_to_canvases_match_oracle",
    # ---- left on the emulator
    "test_pcm16::test_emu_ei_call_runs_again_with_full_tables":
        "emulator only: its SDV_P16_HINT_SKEW hook is compiled under SDV_EMU and the product reads no environment; test_gpu_long_ei_tape_in_calls_matches_oracle "
        "has the call run again on a tape that causes it by itself",
    "test_pcm16::test_emu_burst_counters_as_mask_arithmetic": "emulator only: it calls sdv_emu_selftest_bursts, a symbol of the emulator build",
    # refusals that are decided only after kernels have written into the caller's buffers (inside their stated capacity): nothing is made to run on the
    # GPU for the sake of a refusal unless the code shows that it comes first
    "test_stitch_kernel::test_emu_pipelined_call_reports_what_the_host_would_have_refused":
        "emulator only: the refusal (stitch_engine.inc:482) is decided behind the read-back of a pipelined round whose turn kernel has already written the "
        "caller's buffers (direct_pairs = out_pairs, stitch_engine.inc:405-407)",
    "test_pcm1::test_emu_refuses_what_the_reference_never_finishes":
        "emulator only: FE_FOREIGN is read back (pcm1_engine.inc:111, :122; stitch_stream.inc, read_tail) after the frame kernel has written pairs and descriptors to the caller (:95-99)",
    "test_pcm16::test_emu_refuses_what_the_reference_never_finishes":
        "emulator only: FE_FOREIGN is read back (pcm16_engine.inc:279, :300; stitch_stream.inc, read_tail) after the emit kernels have written pairs and descriptors to the caller (:268)",
    # argument checks of the per-line entries: host code ahead of any device work, the same in both builds; not among the call-by-call tests twinned so far
    "test_stc_lines::test_emu_lines_refuse_bad_arguments": "emulator only: the checks of sdv_binarize_lines are the host's, ahead of its first launch (engine.inc:510-517)",
    "test_pcm1_front::test_emu_argument_checks": "emulator only: the checks of sdv_pcm1_binarize_lines are the host's, ahead of its launch (check_lines_call, markerless_frames_engine.inc:27-40)",
    "test_pcm16_front::test_emu_lines_argument_checks":
        "emulator only: the checks of sdv_pcm16x0_binarize_lines are the host's, ahead of its launch (check_lines_call, markerless_frames_engine.inc:27-40); the rows nothing is preset for "
        "that follow them are an input like those of test_gpu_lines_match_oracle",
}
NOT_YET_TWINNED = []


def _marks(node, module_marks):
    out = set(module_marks)
    for d in node.decorator_list:
        s = ast.unparse(d)
        if s.startswith("pytest.mark."):
            out.add(s[len("pytest.mark."):].split("(")[0])
    return out


def _body(node):
    """The body function of a test that is nothing but one call of it (behind a docstring, if any): `_body(...)`; else None."""
    stmts = [s for s in node.body if not (isinstance(s, ast.Expr) and isinstance(s.value, ast.Constant) and isinstance(s.value.value, str))]
    if len(stmts) == 1 and isinstance(stmts[0], ast.Expr) and isinstance(stmts[0].value, ast.Call) and isinstance(stmts[0].value.func, ast.Name):
        return stmts[0].value.func.id
    return None


def scan():
    """module -> {test name: (marks, its body function or None)}, and module -> names of its module-level functions that are no tests"""
    tests, helpers = {}, {}
    for path in sorted(glob.glob(os.path.join(HERE, "test_*.py"))):
        mod = os.path.basename(path)[:-3]
        tree = ast.parse(open(path).read())
        module_marks = set()
        for node in tree.body:
            if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == "pytestmark" for t in node.targets):
                module_marks |= {s.strip().split("(")[0] for s in ast.unparse(node.value).replace("[", "").replace("]", "").replace("pytest.mark.", "").split(",")}
        funcs = [n for n in tree.body if isinstance(n, ast.FunctionDef)]
        tests[mod] = {f.name: (_marks(f, module_marks), _body(f)) for f in funcs if f.name.startswith("test_")}
        helpers[mod] = {f.name for f in funcs if not f.name.startswith("test_")}
    return tests, helpers


def classify():
    """-> (kind of every test_emu_*: {"module::name": "a" / "b" / "c"}, list of complaints)"""
    tests, helpers = scan()
    kinds, bad = {}, []
    for mod, ts in tests.items():
        for name, (marks, body) in ts.items():
            if not name.startswith("test_emu_"):
                continue
            tid = "%s::%s" % (mod, name)
            entry = COVERED_BY.get(tid)
            twin = "test_gpu_" + name[len("test_emu_"):]
            if tid in NOT_YET_TWINNED:
                if entry is not None:
                    bad.append("%s is in COVERED_BY and in NOT_YET_TWINNED" % tid)
                if mod != "test_emu_parity":
                    bad.append("%s: NOT_YET_TWINNED is for tests/test_emu_parity.py only" % tid)
                kinds[tid] = "open"
            elif entry is not None and entry.startswith("emulator only: "):
                if len(entry) < len("emulator only: ") + 20:
                    bad.append("%s: say why it stays on the emulator" % tid)
                kinds[tid] = "c"
            elif entry is not None:
                m, _, n = entry.partition("::")
                if n not in tests.get(m, {}):
                    bad.append("%s: COVERED_BY names %s, which does not exist" % (tid, entry))
                elif "gpu" not in tests[m][n][0]:
                    bad.append("%s: COVERED_BY names %s, which is not marked gpu" % (tid, entry))
                kinds[tid] = "b"
            elif twin in ts:
                if "gpu" not in ts[twin][0]:
                    bad.append("%s: %s is not marked gpu" % (tid, twin))
                elif body is None or body != ts[twin][1] or body not in helpers[mod]:
                    # the converse: a pair by name is one body called twice, or COVERED_BY says on purpose that the GPU test is written on its own
                    bad.append("%s and %s are not one call of the same body function each: the pair can drift apart (or name the GPU test in COVERED_BY)" % (tid, twin))
                kinds[tid] = "a"
            else:
                bad.append("%s has no GPU twin: add %s calling the same body, or an entry in COVERED_BY" % (tid, twin))
    for tid in list(COVERED_BY) + NOT_YET_TWINNED:
        m, _, n = tid.partition("::")
        if n not in tests.get(m, {}):
            bad.append("%s is listed here but is no test" % tid)
    return kinds, bad


def test_every_emulator_test_has_a_gpu_twin():
    kinds, bad = classify()
    print("test_emu_* by kind: %s" % {k: sum(1 for v in kinds.values() if v == k) for k in ("a", "b", "c", "open")})
    print("NOT_YET_TWINNED:\n  " + "\n  ".join(NOT_YET_TWINNED))
    assert not bad, "\n" + "\n".join(bad)
    assert NOT_YET_TWINNED == [] and "open" not in kinds.values(), "every emulator test has its GPU twin or its reason: the list stays empty"


def test_the_guard_sees_what_it_should():
    """The scanner on sources of its own: marks from decorators and from pytestmark, a pair that shares its body and one that does not."""
    tests, helpers = scan()
    assert "gpu" in tests["test_gpu_parity"]["test_hip_ragged_geometry"][0]                     # pytestmark = pytest.mark.gpu
    assert "gpu" in tests["test_resample"]["test_gpu_refusals"][0] and "gpu" not in tests["test_resample"]["test_emu_refusals"][0]
    assert tests["test_resample"]["test_emu_refusals"][1] == tests["test_resample"]["test_gpu_refusals"][1] == "_refusals" and "_refusals" in helpers["test_resample"]
    assert tests["test_pcm1"]["test_emu_matches_oracle"][1] is None                             # (written out, not one call of a body)
    kinds, _ = classify()
    assert kinds["test_resample::test_emu_refusals"] == "a" and kinds["test_emu_parity::test_emu_bad_arguments"] == "b"
    assert kinds["test_pcm16::test_emu_burst_counters_as_mask_arithmetic"] == "c"


def test_the_guard_of_a_device_buffer_tells():
    """device_calls.DevBuf on the CPU (the same torch code): untouched, it hands out what the call wrote; a byte behind the stated capacity - in the
    room a call with the usual capacity would have had, or in the guard records behind that - fails the check."""
    import numpy as np
    import pytest
    import device_calls as dc
    for at in (4 * 4, 10 * 4 + 7, (10 + dc.GUARD) * 4 - 1):
        b = dc.DevBuf(4, np.uint32, full=10, device="cpu")
        assert len(b) == 4 and b.t.numel() == (10 + dc.GUARD) * 4
        b.t[:16] = 7
        assert b.get().view(np.uint8).tolist() == [7] * 16 and b.get(2, at=1).tolist() == [0x07070707] * 2
        b.t[at] = 0
        with pytest.raises(AssertionError, match="behind the stated capacity"):
            b.get()
        with pytest.raises(AssertionError, match="behind the stated capacity"):
            b.check()
    src = dc.DevBuf(3, np.uint16, data=np.array([1, 2, 3], dtype=np.uint16), device="cpu")
    assert src.get().tolist() == [1, 2, 3] and dc.DevBuf(0, np.uint8, device="cpu").get().size == 0
