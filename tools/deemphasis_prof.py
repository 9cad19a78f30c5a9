"""sdv_audio_deemphasis against a device-to-device copy of the same bytes (both move 12 B in and 12 B out per pair): 14.7 M resident
pairs - BASELINE's 10 000 frames - timed between HIP events on one stream, after a warm-up, in one process.
usage: deemphasis_prof.py [n_pairs] [reps]     -> one JSON line (profiles/deemphasis_notes.md quotes it)"""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdvpcmdecoder_amd import Engine, PAIR_DTYPE  # noqa: E402
from sdvpcmdecoder_amd.engine import DEEMPH_AUTO, DEEMPH_FORCE  # noqa: E402


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps):
        t0.record(); fn(); t1.record(); t1.synchronize()
        times.append(t0.elapsed_time(t1))
    return float(np.median(times)), float(np.min(times))


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 14_700_000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    rng = np.random.default_rng(1)
    a = np.zeros(n, dtype=PAIR_DTYPE)
    a["audio_word"] = rng.integers(-32768, 32768, (n, 2))
    a["sample_flags"] = 3
    a["sample_rate"] = 44056
    src = torch.from_numpy(a.view(np.uint8).reshape(n, 12)).cuda()
    dst = torch.empty_like(src)
    eng = Engine(0)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    stream = torch.cuda.current_stream()
    sptr = C.c_void_p(stream.cuda_stream)

    def copy():
        assert hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), n * 12, 3, sptr) == 0        # hipMemcpyDeviceToDevice

    res = {"n_pairs": n, "bytes_each_way": n * 12, "reps": reps, "device": torch.cuda.get_device_name(0)}
    res["copy_ms"], res["copy_ms_min"] = timed(copy, reps)
    eng.set_deemphasis(DEEMPH_FORCE)
    res["force_ms"], res["force_ms_min"] = timed(lambda: eng.audio_deemphasis(src, out=dst, stream=stream), reps)
    work = src.clone()
    res["force_in_place_ms"], res["force_in_place_ms_min"] = timed(lambda: eng.audio_deemphasis(work, out=work, stream=stream), reps)
    eng.set_deemphasis(DEEMPH_AUTO)         # no pair carries the flag: the kernels' memory traffic without the arithmetic's results
    res["auto_nothing_selected_ms"], res["auto_nothing_selected_ms_min"] = timed(lambda: eng.audio_deemphasis(src, out=dst, stream=stream), reps)
    assert dst.cpu().numpy().tobytes() == a.tobytes()
    res["copy_GBps"] = 2 * n * 12 / res["copy_ms"] / 1e6
    res["force_GBps"] = 2 * n * 12 / res["force_ms"] / 1e6
    res["force_over_copy"] = res["force_ms"] / res["copy_ms"]
    res["force_in_place_over_copy"] = res["force_in_place_ms"] / res["copy_ms"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
