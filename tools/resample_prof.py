"""sdv_audio_resample against a device-to-device copy of the same bytes and against sdv_audio_deemphasis FORCE: 14.7 M resident pairs -
BASELINE's 10 000 NTSC frames, one 44 056 Hz segment - timed between HIP events on one stream, 3 calls of warm-up, median of 20, in one process.
usage: resample_prof.py [n_pairs] [reps] [--notes FILE]
  -> one JSON line; with --notes (profiles/resample_notes.md) the lines of FILE between the two `resample_prof` marker comments are replaced
     by a table of the times and that JSON line.  What the times mean stays prose in the notes, written by whoever ran the tool."""
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


BEGIN, END = "<!-- resample_prof: begin -->", "<!-- resample_prof: end -->"


def write_notes(path, res):
    text = open(path).read()
    head, rest = text.split(BEGIN, 1)
    tail = rest.split(END, 1)[1]
    rows = [("device-to-device copy of the input bytes", "copy_ms"), ("`sdv_audio_deemphasis` FORCE", "deemph_force_ms"),
            ("`sdv_audio_resample`, one segment, flush", "resample_ms"), ("`sdv_audio_resample`, a tag every 1470 pairs, flush", "resample_tagged_ms")]
    body = ["", "%s (%s, %d CUs), %d pairs resident (%d B in), %d outputs; HIP events on one stream, 3 calls of warm-up, %d timed calls:"
            % (res["device"], res["arch"], res["cus"], res["n_pairs"], res["bytes_in"], res["n_out"], res["reps"]), "",
            "| call | median ms | min ms | over the copy |", "|---|---|---|---|"]
    body += ["| %s | %.3f | %.3f | %.2f |" % (name, res[k], res[k + "_min"], res[k] / res["copy_ms"]) for name, k in rows]
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
    a = np.zeros(n, dtype=PAIR_DTYPE)
    a["audio_word"] = rng.integers(-32768, 32768, (n, 2))
    a["sample_flags"] = 3
    a["sample_rate"] = 44056
    src = torch.from_numpy(a.view(np.uint8).reshape(n, 12)).cuda()
    eng = Engine(0)
    eng.set_resample(RESAMPLE_TO_44100)
    room = int(eng.lib.sdv_audio_resample_room(eng._h, n))
    dst = torch.empty((room, 12), dtype=torch.uint8, device="cuda")
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    stream = torch.cuda.current_stream()
    sptr = C.c_void_p(stream.cuda_stream)

    def copy():
        assert hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), n * 12, 3, sptr) == 0        # hipMemcpyDeviceToDevice

    res = {"n_pairs": n, "bytes_in": n * 12, "reps": reps, "device": torch.cuda.get_device_name(0),
           "arch": torch.cuda.get_device_properties(0).gcnArchName, "cus": torch.cuda.get_device_properties(0).multi_processor_count}
    res["copy_ms"], res["copy_ms_min"] = timed(copy, reps)
    eng.set_deemphasis(DEEMPH_FORCE)
    res["deemph_force_ms"], res["deemph_force_ms_min"] = timed(lambda: eng.audio_deemphasis(src, out=dst, stream=stream), reps)
    got = []
    res["resample_ms"], res["resample_ms_min"] = timed(lambda: got.append(eng.audio_resample(src, flush=True, out=dst, stream=stream).shape[0]), reps)
    assert set(got) == {(n - 1) * 1001 // 1000 + 1}
    res["n_out"] = got[0]
    # the same stream with a tag every 1470 pairs (a segment per frame): what the boundaries cost
    a["service_type"][::1470] = 1
    src.copy_(torch.from_numpy(a.view(np.uint8).reshape(n, 12)))
    res["resample_tagged_ms"], res["resample_tagged_ms_min"] = timed(lambda: eng.audio_resample(src, flush=True, out=dst, stream=stream), reps)
    res["resample_over_copy"] = res["resample_ms"] / res["copy_ms"]
    res["resample_over_deemph"] = res["resample_ms"] / res["deemph_force_ms"]
    res["fp64_gflops"] = 2 * 2 * 128 * res["n_out"] / res["resample_ms"] / 1e6
    res["tap_bytes_GBps"] = 128 * 8 * res["n_out"] / res["resample_ms"] / 1e6
    print(json.dumps(res))
    if notes:
        write_notes(notes, res)


if __name__ == "__main__":
    main()
