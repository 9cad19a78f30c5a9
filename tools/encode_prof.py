"""sdv_encode_frames against a hipMemsetAsync of the bytes it writes (the floor of a write-only pass) and against synth.stc007_frames_torch, which
made such batches until now: BASELINE's batch of 10 000 NTSC frames (720 x 486), 14 bit with the control block, resident; timed between HIP events
on the engine's stream, 3 calls of warm-up, median of 20, the calls of a comparison alternating in one process.
usage: encode_prof.py [n_frames] [reps] [--out FILE] [--markerless all|pcm1,pcm16x0_si,pcm16x0_ei] [--pix all|uyvy422,v210,...]
  -> one JSON line (also written to FILE).  What the figures mean is prose in profiles/encode_notes.md, written by whoever ran the tool.
With --markerless: sdv_encode_markerless_frames for the formats named (PCM-1 with one Header line) beside sdv_encode_frames at the same geometry,
720 x 490, the same method, all alternating in one process; every call's words step from a call with a picture of 1 x 1.
With --pix: sdv_encode_frames with out_fmt set to each of the packed formats named (all: uyvy422, v210, gray10le, rgb24, rgb0), each beside a
hipMemsetAsync of the bytes that format writes, the SDV_PIX_GRAY8 call of the same run and the uyvy422 call with the destination 3 bytes off, the same
method, all alternating in one process.  A two-pass design pays at least the GRAY8 call plus a fill of the packed bytes: `*_bar_ms` is that sum.
The share of the raster kernel is taken from a call with the same frames and a picture of 1 x 1: its words step is the same, its raster step is
10 000 bytes."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdvpcmdecoder_amd import Engine, EncodeDesc, EncodeMarkerlessDesc, synth  # noqa: E402
from sdvpcmdecoder_amd.abi import PIX_FORMATS  # noqa: E402

W, H = 720, 486


def timed(fns, reps, warmup=3):
    """the calls of `fns` in turn, reps times -> [(median ms, min ms)] in their order"""
    for _ in range(warmup):
        for fn in fns:
            fn()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            t0.record(); fn(); t1.record(); t1.synchronize()
            times[k].append(t0.elapsed_time(t1))
    return [(float(np.median(t)), float(np.min(t))) for t in times]


def main():
    argv = sys.argv[1:]
    out_path = None
    if "--out" in argv:
        at = argv.index("--out")
        out_path = argv[at + 1]
        del argv[at:at + 2]
    formats = []
    if "--markerless" in argv:
        at = argv.index("--markerless")
        formats = ["pcm1", "pcm16x0_si", "pcm16x0_ei"] if argv[at + 1] == "all" else argv[at + 1].split(",")
        del argv[at:at + 2]
    pix = []
    if "--pix" in argv:
        at = argv.index("--pix")
        pix = ["uyvy422", "v210", "gray10le", "rgb24", "rgb0"] if argv[at + 1] == "all" else argv[at + 1].split(",")
        del argv[at:at + 2]
    n = int(argv[0]) if len(argv) > 0 else 10_000
    reps = int(argv[1]) if len(argv) > 1 else 20
    eng = Engine(0)
    lib, h = eng.lib, eng._h
    sptr = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    nbytes = n * H * W
    pcm = torch.randint(-32768, 32768, (n * 1470, 2), dtype=torch.int16, device="cuda")
    row_bytes = {nm: eng.encode_geometry(EncodeDesc(0, 0, 1, 0, 0, 30, 200, 0, 0, 0, 0, 0, 0, (C.c_uint8 * 3)(PIX_FORMATS[nm]), W, H, 12, 708, 2))[2] for nm in pix}
    dst = torch.empty(n * 490 * max([W] + list(row_bytes.values())) + 64, dtype=torch.uint8, device="cuda")     # (room for the 490 rows of --markerless, the widest rows of --pix)

    # what it makes is what the repository's generator makes: two frames without the control block against synth.stc007_frames on the same words
    two = eng.encode_frames(pcm[:2 * 1470], 2, height=H, top_line=2).cpu().numpy()
    words = (pcm[:2 * 1470].cpu().numpy().view(np.uint16).reshape(-1, 6) >> 2).astype(np.uint32)
    assert np.array_equal(two, synth.stc007_frames(2, audio=words, height=H, cut_top=2)[0])
    eng.reset_encoder()

    def encode(width=W, height=H, at=0, out_fmt=0):
        d = EncodeDesc(0, 0, 1, 0, 0, 30, 200, 0, 0, 0, 0, 0, 0, (C.c_uint8 * 3)(out_fmt), width, height, 12, 708, 2)
        rb = eng.encode_geometry(d)[2]

        def fn():
            rc = lib.sdv_encode_frames(h, C.byref(d), C.c_void_p(pcm.data_ptr()), n * 1470, n, C.c_void_p(dst.data_ptr() + at), rb, rb * height, sptr)
            assert rc == 0, lib.sdv_last_error(h)
        return fn

    def fill(count=None):
        assert hip.hipMemsetAsync(dst.data_ptr(), 30, nbytes if count is None else count, sptr) == 0

    def markerless(fmt, width=W, height=490):
        """sdv_encode_markerless_frames: PCM-1 with one Header line, PCM-16x0 with the 44100 bit"""
        d = EncodeMarkerlessDesc(fmt, 0, 30, 200, 1 if fmt == 0 else 0, 0 if fmt == 0 else 2, (C.c_uint8 * 2)(), width, height, 4, 716, 0)

        def fn():
            rc = lib.sdv_encode_markerless_frames(h, C.byref(d), C.c_void_p(pcm.data_ptr()), n * 1470, n, C.c_void_p(dst.data_ptr()), width, width * height, sptr)
            assert rc == 0, lib.sdv_last_error(h)
        return fn

    p = torch.cuda.get_device_properties(0)
    if pix:
        # the packed formats beside the GRAY8 call, each with the fill of its own bytes; uyvy422 also 3 bytes off
        fns, keys = [encode()], ["gray8"]
        for nm in pix:
            fns += [encode(out_fmt=PIX_FORMATS[nm]), (lambda c: lambda: fill(c))(n * H * row_bytes[nm])]
            keys += [nm, nm + "_memset"]
        fns.append(encode(at=3, out_fmt=PIX_FORMATS["uyvy422"]))
        keys.append("uyvy422_dst_plus_3")
        res = {"n_frames": n, "reps": reps, "device": torch.cuda.get_device_name(0), "arch": p.gcnArchName, "cus": p.multi_processor_count, "width": W, "height": H}
        for key, (ms, mn) in zip(keys, timed(fns, reps)):
            res[key + "_ms"], res[key + "_ms_min"] = ms, mn
        for nm in pix:
            res[nm + "_bytes"] = n * H * row_bytes[nm]
            res[nm + "_over_memset"] = res[nm + "_ms"] / res[nm + "_memset_ms"]
            res[nm + "_bar_ms"] = res["gray8_ms"] + res[nm + "_memset_ms"]
            res[nm + "_below_bar"] = res[nm + "_ms"] < res[nm + "_bar_ms"]
        line = json.dumps(res)
        print(line)
        if out_path:
            os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
            open(out_path, "w").write(line + "\n")
        return
    if formats:
        # the marker-less formats beside sdv_encode_frames at the same geometry, 720 x 490, all alternating in one process; the words step of each
        # from a call with a picture of 1 x 1
        names = {"pcm1": 0, "pcm16x0_si": 1, "pcm16x0_ei": 2}
        nbytes = n * 490 * W
        fns, keys = [encode(height=490), encode(1, 1)], ["encode", "encode_words_only"]
        for nm in formats:
            fns += [markerless(names[nm]), markerless(names[nm], 1, 1)]
            keys += [nm, nm + "_words_only"]
        res = {"n_frames": n, "reps": reps, "device": torch.cuda.get_device_name(0), "arch": p.gcnArchName, "cus": p.multi_processor_count, "bytes": nbytes,
               "width": W, "height": 490}
        for key, (ms, mn) in zip(keys, timed(fns, reps)):
            res[key + "_ms"], res[key + "_ms_min"] = ms, mn
        for nm in formats:
            res[nm + "_over_encode"] = res[nm + "_ms"] / res["encode_ms"]
            res[nm + "_raster_share"] = 1.0 - res[nm + "_words_only_ms"] / res[nm + "_ms"]
        line = json.dumps(res)
        print(line)
        if out_path:
            os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
            open(out_path, "w").write(line + "\n")
        return
    res = {"n_frames": n, "reps": reps, "device": torch.cuda.get_device_name(0), "arch": p.gcnArchName, "cus": p.multi_processor_count, "bytes": nbytes}
    (e_ms, e_min), (f_ms, f_min), (w_ms, w_min), (m_ms, m_min) = timed([encode(), fill, encode(1, 1), encode(at=3)], reps)
    res.update({"encode_ms": e_ms, "encode_ms_min": e_min, "encode_gbps": nbytes / e_ms / 1e6, "memset_ms": f_ms, "memset_ms_min": f_min,
                "memset_gbps": nbytes / f_ms / 1e6, "encode_over_memset": e_ms / f_ms, "words_only_ms": w_ms, "words_only_ms_min": w_min,
                "raster_share": 1.0 - w_ms / e_ms, "raster_over_memset": (e_ms - w_ms) / f_ms,
                "dst_plus_3_ms": m_ms, "dst_plus_3_ms_min": m_min, "dst_plus_3_over_aligned": m_ms / e_ms})
    del dst
    torch.cuda.empty_cache()
    # the generator of the benchmark's batch, on the same box: once at 256 frames to warm it up, then the whole tape against a host clock
    synth.stc007_frames_torch(256, seed=1)
    torch.cuda.synchronize()
    times = []
    for _ in range(2):
        t0 = time.perf_counter()
        luma, _ = synth.stc007_frames_torch(n, seed=1)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
        del luma
    res.update({"synth_torch_ms": min(times), "synth_torch_over_encode": min(times) / e_ms})
    line = json.dumps(res)
    print(line)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        open(out_path, "w").write(line + "\n")


if __name__ == "__main__":
    main()
