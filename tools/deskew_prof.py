"""The skew stage of sdv_audio_resample (SDV_RESAMPLE_DELAY_RIGHT, mode 4) against a device-to-device copy of the same pairs, against
sdv_audio_deemphasis FORCE, and behind the resampler (mode 5) against the resampler alone (mode 1) plus the stage alone: 14.7 M resident pairs -
BASELINE's 10 000 NTSC frames, one segment, flush - timed between HIP events on one stream, 3 calls of warm-up, median of 20, in one process; the
calls take turns, round by round, so that a drift of the clock meets all of them.
usage: deskew_prof.py [n_pairs] [reps] [--notes FILE] [--json FILE]
  -> one JSON line (also written to --json FILE); with --notes (profiles/deskew_notes.md) the lines of FILE between the two `deskew_prof` marker
     comments are replaced by a table of the times and that JSON line.  What the times mean stays prose in the notes, written by whoever ran the tool.
With SDVPCM_LIB set to a build from before the stage the modes 4 and 5 are left out (null): mode 1 of two builds in two runs of this tool."""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdvpcmdecoder_amd import Engine, PAIR_DTYPE  # noqa: E402
from sdvpcmdecoder_amd.engine import DEEMPH_FORCE, RESAMPLE_TO_44100  # noqa: E402

DELAY_RIGHT = 4

BEGIN, END = "<!-- deskew_prof: begin -->", "<!-- deskew_prof: end -->"
ROWS = [("device-to-device copy of the pairs (12 B a pair)", "copy"), ("`sdv_audio_deemphasis` FORCE", "deemph_force"),
        ("`sdv_audio_resample` mode 4 (copy + skew stage)", "mode4"), ("`sdv_audio_resample` mode 1 (resampler)", "mode1"),
        ("`sdv_audio_resample` mode 5 (resampler + skew stage)", "mode5")]


def write_notes(path, res):
    text = open(path).read()
    head, rest = text.split(BEGIN, 1)
    tail = rest.split(END, 1)[1]
    body = ["", "%s (%s, %d CUs), %d pairs resident; HIP events on one stream, 3 calls of warm-up, %d timed rounds in which the calls take turns:"
            % (res["device"], res["arch"], res["cus"], res["n_pairs"], res["reps"]), "",
            "| call | median ms | min ms | max ms | over the copy |", "|---|---|---|---|---|"]
    body += ["| %s | %.3f | %.3f | %.3f | %.2f |" % (name, res[k + "_ms"], res[k + "_ms_min"], res[k + "_ms_max"], res[k + "_ms"] / res["copy_ms"])
             for name, k in ROWS if res.get(k + "_ms") is not None]
    body += ["", "```json", json.dumps(res), "```", ""]
    open(path, "w").write(head + BEGIN + "\n".join(body) + END + tail)


def main():
    argv = sys.argv[1:]
    opts = {}
    for name in ("--notes", "--json"):
        if name in argv:
            at = argv.index(name)
            opts[name] = argv[at + 1]
            del argv[at:at + 2]
    n = int(argv[0]) if len(argv) > 0 else 14_700_000
    reps = int(argv[1]) if len(argv) > 1 else 20
    rng = np.random.default_rng(1)
    a = np.zeros(n, dtype=PAIR_DTYPE)
    a["audio_word"] = rng.integers(-8000, 8001, (n, 2)).astype(np.int16)
    a["sample_flags"] = 3
    a["sample_rate"] = 44056
    pairs = torch.from_numpy(a.view(np.uint8).reshape(n, 12)).cuda()
    del a
    eng = Engine(0)
    eng.set_deemphasis(DEEMPH_FORCE)
    eng.set_resample(RESAMPLE_TO_44100)
    room = int(eng.lib.sdv_audio_resample_room(eng._h, n)) + 64
    pairs_out = torch.empty((room, 12), dtype=torch.uint8, device="cuda")
    has_stage = eng.lib.sdv_set_resample(eng._h, DELAY_RIGHT) == 0
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    stream = torch.cuda.current_stream()
    sptr = C.c_void_p(stream.cuda_stream)
    counts = {}

    def copy():
        assert hip.hipMemcpyAsync(pairs_out.data_ptr(), pairs.data_ptr(), n * 12, 3, sptr) == 0         # hipMemcpyDeviceToDevice

    def mode(m):
        def call():
            eng.set_resample(m)
            counts.setdefault(m, set()).add(eng.audio_resample(pairs, flush=True, out=pairs_out, stream=stream).shape[0])
        return call

    calls = [("copy", copy), ("deemph_force", lambda: eng.audio_deemphasis(pairs, out=pairs_out, stream=stream)), ("mode1", mode(RESAMPLE_TO_44100))]
    if has_stage:
        calls += [("mode4", mode(DELAY_RIGHT)), ("mode5", mode(RESAMPLE_TO_44100 | DELAY_RIGHT))]
    times = {k: [] for k, _ in calls}
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for r in range(3 + reps):
        for k, fn in calls:
            t0.record(); fn(); t1.record(); t1.synchronize()
            if r >= 3:
                times[k].append(t0.elapsed_time(t1))
    res = {"n_pairs": n, "bytes_pairs": n * 12, "reps": reps, "device": torch.cuda.get_device_name(0), "lib": os.environ.get("SDVPCM_LIB", "the package's"),
           "arch": torch.cuda.get_device_properties(0).gcnArchName, "cus": torch.cuda.get_device_properties(0).multi_processor_count}
    for _, k in ROWS:
        t = times.get(k)
        res[k + "_ms"], res[k + "_ms_min"], res[k + "_ms_max"] = (float(np.median(t)), float(np.min(t)), float(np.max(t))) if t else (None, None, None)
    n_res = (n - 1) * 1001 // 1000 + 1
    assert counts[RESAMPLE_TO_44100] == {n_res}
    if has_stage:
        assert counts[DELAY_RIGHT] == {n} and counts[RESAMPLE_TO_44100 | DELAY_RIGHT] == {n_res}
        res["mode4_over_copy"] = res["mode4_ms"] / res["copy_ms"]
        res["mode4_over_deemph"] = res["mode4_ms"] / res["deemph_force_ms"]
        res["mode5_over_mode1_plus_mode4"] = res["mode5_ms"] / (res["mode1_ms"] + res["mode4_ms"])
        res["mode4_GBps"] = 2 * 12 * n / res["mode4_ms"] / 1e6
        res["mode4_fp64_gflops"] = 2 * 128 * n / res["mode4_ms"] / 1e6
    print(json.dumps(res))
    if "--json" in opts:
        os.makedirs(os.path.dirname(os.path.abspath(opts["--json"])), exist_ok=True)
        open(opts["--json"], "w").write(json.dumps(res) + "\n")
    if "--notes" in opts:
        write_notes(opts["--notes"], res)


if __name__ == "__main__":
    main()
