#!/usr/bin/env python3
"""sdv_audio_process timed with HIP events in one process, for profiles/conceal_notes.md: SDV_DROP_INTER_LIN_WORD (6) and SDV_DROP_INTER_CUBIC_WORD (9) of
this build and, given a library built from another commit, mode 6 of that one, the calls taking turns round by round (who goes first moves on with the
round), on the three audio tapes of bench.py --full: clean, a dropout every 25 frames, an invalid word in every window.
    tools/conceal_prof.py [n_frames] [other libsdvpcm_hip.so] [result.json]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_FRAMES = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
OTHER = sys.argv[2] if len(sys.argv) > 2 else None
RESULT = sys.argv[3] if len(sys.argv) > 3 else None
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import audio_api as A
from sdvpcmdecoder_amd import abi, load_library

ROUNDS, WARM = 21, 3
torch.cuda.init()
dev = torch.device("cuda:0")
new = abi.bind(C.CDLL(load_library()._name))
old = abi.bind(C.CDLL(OTHER)) if OTHER else None
e_new, e_old = new.sdv_engine_create(0), old.sdv_engine_create(0) if old else None
assert e_new and (e_old or not old)

npairs = N_FRAMES * 1470
rng = np.random.default_rng(9)
starts = np.sort(rng.integers(1000, npairs - 5000, max(1, N_FRAMES // 25)))
tapes = (("clean", dict()),
         ("dropout_every_25_frames", dict(runs=[(int(s_), int(rng.integers(1, 700)), int(rng.integers(0, 3))) for s_ in starts])),
         ("invalid_word_in_every_window", dict(p_bad=0.01)))
out = torch.empty((npairs + 1024, 12), dtype=torch.uint8, device=dev)
pur = torch.empty((16, 16), dtype=torch.uint8, device=dev)
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)


def call(lib, eng, mode, d_t, n):
    assert lib.sdv_set_audio_masking(eng, mode) == 0 and lib.sdv_reset_audio(eng) == 0
    n_out, n_pur, nm = C.c_size_t(0), C.c_size_t(0), C.c_uint64(0)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    rc = lib.sdv_audio_process(eng, d_t.data_ptr(), n, 1, out.data_ptr(), npairs + 1024, C.byref(n_out), pur.data_ptr(), 16, C.byref(n_pur), C.byref(nm), stream)
    b.record()
    torch.cuda.synchronize(dev)
    assert rc == 0, lib.sdv_last_error(eng)
    return a.elapsed_time(b), n_out.value, nm.value


result = {"pairs": npairs, "rounds": ROUNDS, "warm_up": WARM, "device": torch.cuda.get_device_name(0), "abi": [new.sdv_abi_version(), old.sdv_abi_version() if old else None], "tapes": {}}
t_start = time.time()
for name, kw in tapes:
    tape = A.tape(["N", A.audio(npairs, 3, tone=False, **kw), "E"])
    d_t = torch.from_numpy(tape.view(np.uint8).reshape(len(tape), 12)).to(dev)
    variants = ((("other_mode6", old, e_old, 6),) if old else ()) + (("this_mode6", new, e_new, 6), ("this_mode9", new, e_new, 9))
    ms = {v[0]: [] for v in variants}
    masked, sums = {}, {}
    for r in range(WARM + ROUNDS):
        for vname, lib, eng, mode in variants[r % len(variants):] + variants[:r % len(variants)]:
            t, n_out, nm = call(lib, eng, mode, d_t, len(tape))
            if r >= WARM:
                ms[vname].append(t)
            if r == 0:
                masked[vname] = nm
                sums[vname] = int(out[:n_out].to(torch.int64).sum().item())
    assert not old or (sums["other_mode6"] == sums["this_mode6"] and masked["other_mode6"] == masked["this_mode6"]), "mode 6 differs from the other library's"
    row = {"masked": masked}
    for vname in ms:
        x = np.sort(np.array(ms[vname]))
        row[vname] = {"median_ms": float(np.median(x)), "min_ms": float(x[0]), "max_ms": float(x[-1]), "q1_ms": float(x[len(x) // 4]), "q3_ms": float(x[(3 * len(x)) // 4])}
    result["tapes"][name] = row
    print(name, json.dumps(row), flush=True)
    del d_t
result["wall_s"] = time.time() - t_start
if RESULT:
    json.dump(result, open(RESULT, "w"), indent=1)
new.sdv_engine_destroy(e_new)
if old:
    old.sdv_engine_destroy(e_old)
