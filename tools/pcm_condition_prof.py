"""sdv_pcm_preemphasis and sdv_pcm_resample against a device-to-device copy of their input bytes and against their decode-side twins,
sdv_audio_deemphasis FORCE and sdv_audio_resample (one segment, flush), on the same number of pairs: 14.7 M resident pairs - BASELINE's 10 000
NTSC frames - timed between HIP events on one stream, 3 calls of warm-up, median of 20, in one process.
usage: pcm_condition_prof.py [n_pairs] [reps] [--notes FILE]
  -> one JSON line; with --notes (profiles/pcm_condition_notes.md) the lines of FILE between the two `pcm_condition_prof` marker comments are
     replaced by a table of the times and that JSON line.  What the times mean stays prose in the notes, written by whoever ran the tool."""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdvpcmdecoder_amd import Engine, PAIR_DTYPE  # noqa: E402
from sdvpcmdecoder_amd.engine import DEEMPH_FORCE, RESAMPLE_TO_44100  # noqa: E402


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps):
        t0.record(); fn(); t1.record(); t1.synchronize()
        times.append(t0.elapsed_time(t1))
    return float(np.median(times)), float(np.min(times))


BEGIN, END = "<!-- pcm_condition_prof: begin -->", "<!-- pcm_condition_prof: end -->"
ROWS = [("device-to-device copy of the PCM bytes (4 B a pair)", "copy_ms"), ("`sdv_pcm_preemphasis`", "preemph_ms"),
        ("`sdv_audio_deemphasis` FORCE (12 B a pair)", "deemph_force_ms"), ("`sdv_pcm_resample`, flush", "pcm_resample_ms"),
        ("`sdv_audio_resample`, one segment, flush (12 B a pair)", "audio_resample_ms")]


def write_notes(path, res):
    text = open(path).read()
    head, rest = text.split(BEGIN, 1)
    tail = rest.split(END, 1)[1]
    body = ["", "%s (%s, %d CUs), %d pairs resident; HIP events on one stream, 3 calls of warm-up, %d timed calls:"
            % (res["device"], res["arch"], res["cus"], res["n_pairs"], res["reps"]), "",
            "| call | median ms | min ms | over the copy |", "|---|---|---|---|"]
    body += ["| %s | %.3f | %.3f | %.2f |" % (name, res[k], res[k + "_min"], res[k] / res["copy_ms"]) for name, k in ROWS]
    body += ["", "```json", json.dumps(res), "```", ""]
    open(path, "w").write(head + BEGIN + "\n".join(body) + END + tail)


def main():
    argv = sys.argv[1:]
    notes = None
    if "--notes" in argv:
        at = argv.index("--notes")
        notes = argv[at + 1]
        del argv[at:at + 2]
    n = int(argv[0]) if len(argv) > 0 else 14_700_000
    reps = int(argv[1]) if len(argv) > 1 else 20
    rng = np.random.default_rng(1)
    words = rng.integers(-8000, 8001, (n, 2)).astype(np.int16)
    pcm = torch.from_numpy(words).cuda()
    pcm_out = torch.empty((n + 16, 2), dtype=torch.int16, device="cuda")
    a = np.zeros(n, dtype=PAIR_DTYPE)
    a["audio_word"] = words
    a["sample_flags"] = 3
    a["sample_rate"] = 44056
    pairs = torch.from_numpy(a.view(np.uint8).reshape(n, 12)).cuda()
    del a
    eng = Engine(0)
    eng.set_resample(RESAMPLE_TO_44100)
    eng.set_deemphasis(DEEMPH_FORCE)
    pairs_out = torch.empty((int(eng.lib.sdv_audio_resample_room(eng._h, n)), 12), dtype=torch.uint8, device="cuda")
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    stream = torch.cuda.current_stream()
    sptr = C.c_void_p(stream.cuda_stream)

    def copy():
        assert hip.hipMemcpyAsync(pcm_out.data_ptr(), pcm.data_ptr(), n * 4, 3, sptr) == 0          # hipMemcpyDeviceToDevice

    res = {"n_pairs": n, "bytes_pcm": n * 4, "reps": reps, "device": torch.cuda.get_device_name(0),
           "arch": torch.cuda.get_device_properties(0).gcnArchName, "cus": torch.cuda.get_device_properties(0).multi_processor_count}
    res["copy_ms"], res["copy_ms_min"] = timed(copy, reps)
    res["preemph_ms"], res["preemph_ms_min"] = timed(lambda: eng.pcm_preemphasis(pcm, 44056, out=pcm_out, stream=stream), reps)
    res["preemph_clipped"] = eng.preemphasis_clipped(stream)
    res["deemph_force_ms"], res["deemph_force_ms_min"] = timed(lambda: eng.audio_deemphasis(pairs, out=pairs_out, stream=stream), reps)
    got = []
    res["pcm_resample_ms"], res["pcm_resample_ms_min"] = timed(lambda: got.append(eng.pcm_resample(pcm, flush=True, out=pcm_out, stream=stream).shape[0]), reps)
    assert set(got) == {(1000 * n - 1) // 1001 + 1}
    res["pcm_resample_n_out"] = got[0]
    got = []
    res["audio_resample_ms"], res["audio_resample_ms_min"] = timed(lambda: got.append(eng.audio_resample(pairs, flush=True, out=pairs_out, stream=stream).shape[0]), reps)
    assert set(got) == {(n - 1) * 1001 // 1000 + 1}
    res["audio_resample_n_out"] = got[0]
    res["preemph_over_deemph"] = res["preemph_ms"] / res["deemph_force_ms"]
    res["pcm_resample_over_audio_resample"] = res["pcm_resample_ms"] / res["audio_resample_ms"]
    res["preemph_GBps"] = 2 * 4 * n / res["preemph_ms"] / 1e6
    res["pcm_resample_fp64_gflops"] = 2 * 2 * 128 * res["pcm_resample_n_out"] / res["pcm_resample_ms"] / 1e6
    res["pcm_resample_tap_bytes_GBps"] = 128 * 8 * res["pcm_resample_n_out"] / 4 / res["pcm_resample_ms"] / 1e6      # a tap is loaded once for four outputs
    print(json.dumps(res))
    if notes:
        write_notes(notes, res)


if __name__ == "__main__":
    main()
