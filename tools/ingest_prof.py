"""sdv_ingest_frames against a device-to-device copy that moves the same bytes, against sdv_double_width, and at aligned / misaligned source
addresses: BASELINE's batch of 10 000 NTSC frames (720 x 486), resident; timed between HIP events on one stream, 3 calls of warm-up, median of
20, the calls of a comparison alternating in one process.
usage: ingest_prof.py [n_frames] [reps] [--notes FILE] [--resources REMARKS]
  -> one JSON line; with --notes (profiles/ingest_notes.md) the lines of FILE between the two `ingest_prof` marker comments are replaced by
     tables of the figures and that JSON line.  --resources: hipcc's -Rpass-analysis=kernel-resource-usage remarks of the library's build
     (tools/kernel_resources.py reads them), for the register table.  What the figures mean stays prose in the notes, written by whoever ran
     the tool."""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sdvpcmdecoder_amd import Engine, IngestDesc  # noqa: E402
from sdvpcmdecoder_amd.engine import INGEST_DOUBLE_AUTO, PIX_FORMATS  # noqa: E402

W, H = 720, 486
BEGIN, END = "<!-- ingest_prof: begin -->", "<!-- ingest_prof: end -->"
FAMILIES = ("gray8", "uyvy422", "yuyv422", "v210", "gray10le", "rgb24/bgr24", "rgb0/bgr0")


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


def resources(path):
    """the 14 builds of sdv_k_ingest in the compiler's remarks; a build without its figures is an error, not a row of zeros"""
    import kernel_resources as kr
    out = []
    for name, r in sorted(kr.parse(open(path).read()).items()):
        m = re.match(r"_Z12sdv_k_ingestILi(\d)ELb(\d)E", name)
        if m:
            missing = [k for k in ("vgpr", "sgpr", "scratch", "lds", "occupancy") if k not in r]
            if missing:
                raise SystemExit("%s: no %s for %s (remarks in another format than tools/kernel_resources.py reads?)" % (path, ", ".join(missing), name))
            out.append({"kernel": "sdv_k_ingest<%s, %s>" % (FAMILIES[int(m.group(1))], "doubling" if m.group(2) == "1" else "plain"),
                        "vgpr": r["vgpr"], "sgpr": r["sgpr"], "scratch": r["scratch"], "lds": r["lds"], "occupancy": r["occupancy"]})
    if len(out) != 2 * len(FAMILIES):
        raise SystemExit("%s: %d builds of sdv_k_ingest, %d expected" % (path, len(out), 2 * len(FAMILIES)))
    return out


def write_notes(path, res):
    text = open(path).read()
    head, rest = text.split(BEGIN, 1)
    tail = rest.split(END, 1)[1]
    body = ["", "%s (%s, %d CUs), %d frames of %d x %d resident; HIP events on one stream, 3 calls of warm-up, median of %d timed calls (min in brackets), the calls of a "
            "row alternating:" % (res["device"], res["arch"], res["cus"], res["n_frames"], W, H, res["reps"]), "",
            "**1, 2. Throughput, with doubling (out 1440 x 486), against a `hipMemcpyAsync` device-to-device copy of (read + written) / 2 bytes**", "",
            "| format | read MB | written MB | ingest ms | read + written GB/s | copy ms | copy GB/s | ingest / copy |", "|---|---|---|---|---|---|---|---|"]
    for r in res["throughput"]:
        body.append("| `%s` | %.0f | %.0f | %.3f (%.3f) | %.0f | %.3f (%.3f) | %.0f | %.2f |" % (
            r["fmt"], r["read"] / 1e6, r["written"] / 1e6, r["ingest_ms"], r["ingest_ms_min"], r["gbps"], r["copy_ms"], r["copy_ms_min"], r["copy_gbps"], r["ratio"]))
    d = res["double_width"]
    body += ["", "**3. `GRAY8` + doubling against `sdv_double_width` on the same pixels**", "",
             "| call | ms |", "|---|---|", "| `sdv_ingest_frames` | %.3f (%.3f) |" % (d["ingest_ms"], d["ingest_ms_min"]),
             "| `sdv_double_width` | %.3f (%.3f) |" % (d["double_width_ms"], d["double_width_ms_min"]), "", "ingest / sdv_double_width: %.2f" % d["ratio"]]
    body += ["", "**4. Source alignment, `UYVY422`, 718 pixels kept, destination rows 16-byte aligned (stride 1440)**", "",
             "| source | ms | against aligned |", "|---|---|---|"]
    for r in res["alignment"]:
        body.append("| %s | %.3f (%.3f) | %.2f |" % (r["case"], r["ms"], r["ms_min"], r["ms"] / res["alignment"][0]["ms"]))
    if res.get("resources"):
        body += ["", "**5. Resources (hipcc's -Rpass-analysis=kernel-resource-usage remarks of the library's build for gfx950)**", "", "| kernel | VGPR | SGPR | scratch B/lane | LDS B | waves/SIMD |", "|---|---|---|---|---|---|"]
        body += ["| `%s` | %d | %d | %d | %d | %s |" % (r["kernel"], r["vgpr"], r["sgpr"], r["scratch"], r["lds"], r["occupancy"]) for r in res["resources"]]
    body += ["", "```json", json.dumps(res), "```", ""]
    open(path, "w").write(head + BEGIN + "\n".join(body) + END + tail)


def main():
    argv = sys.argv[1:]
    notes = remarks = None
    for flag in ("--notes", "--resources"):
        if flag in argv:
            at = argv.index(flag)
            if flag == "--notes":
                notes = argv[at + 1]
            else:
                remarks = argv[at + 1]
            del argv[at:at + 2]
    n = int(argv[0]) if len(argv) > 0 else 10_000
    reps = int(argv[1]) if len(argv) > 1 else 20
    eng = Engine(0)
    lib, h = eng.lib, eng._h
    stream = torch.cuda.current_stream()
    sptr = C.c_void_p(stream.cuda_stream)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    res_table = resources(remarks) if remarks else None         # (before any GPU work: a file that does not parse ends the run here)
    rows = n * H
    src = torch.empty(rows * 4 * W + 64, dtype=torch.uint8, device="cuda")         # the largest source (4 bytes a pixel) and room for an offset
    for at in range(0, src.numel(), 1 << 30):
        src[at:at + (1 << 30)].random_(0, 256)
    dst = torch.empty(rows * (4 * W + 2 * W) // 2 + 64, dtype=torch.uint8, device="cuda")      # the largest copy; the planes (2 W a row) fit
    torch.cuda.synchronize()

    def ingest(fmt, crop=(0, 0, 0, 0), src_at=0, dst_stride=None):
        d = IngestDesc(PIX_FORMATS[fmt], 0, INGEST_DOUBLE_AUTO, 0, crop[0], crop[1], crop[2], crop[3], W, H)
        ow, oh, doubled, rb = eng.ingest_geometry(d)
        assert doubled and oh == H
        ds = dst_stride or ow

        def fn():
            rc = lib.sdv_ingest_frames(h, C.byref(d), C.c_void_p(src.data_ptr() + src_at), rb, rb * H, n, C.c_void_p(dst.data_ptr()), ds, ds * H, sptr)
            assert rc == 0, lib.sdv_last_error(h)
        return fn, rows * rb, rows * ow, ow

    def copy(nbytes):
        def fn():
            assert hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, 3, sptr) == 0          # hipMemcpyDeviceToDevice
        return fn

    p = torch.cuda.get_device_properties(0)
    res = {"n_frames": n, "reps": reps, "device": torch.cuda.get_device_name(0), "arch": p.gcnArchName, "cus": p.multi_processor_count, "throughput": []}
    for fmt in ("uyvy422", "v210", "bgr0", "gray8"):
        fn, rd, wr, ow = ingest(fmt)
        fn()
        if fmt in ("uyvy422", "gray8"):             # the first frame against torch's own indexing
            rb = rd // rows
            first = src[:H * rb].view(H, rb)
            want = (first[:, 1::2] if fmt == "uyvy422" else first)[:, :W].repeat_interleave(2, dim=1)
            assert torch.equal(dst[:H * ow].view(H, ow), want)
        (i_ms, i_min), (c_ms, c_min) = timed([fn, copy((rd + wr) // 2)], reps)
        res["throughput"].append({"fmt": fmt, "read": rd, "written": wr, "ingest_ms": i_ms, "ingest_ms_min": i_min, "gbps": (rd + wr) / i_ms / 1e6,
                                  "copy_ms": c_ms, "copy_ms_min": c_min, "copy_gbps": (rd + wr) / c_ms / 1e6, "ratio": i_ms / c_ms})
    fn, _, _, _ = ingest("gray8")

    def double_width():
        rc = lib.sdv_double_width(h, C.c_void_p(src.data_ptr()), W, W, rows, C.c_void_p(dst.data_ptr()), 2 * W, sptr)
        assert rc == 0, lib.sdv_last_error(h)
    (i_ms, i_min), (d_ms, d_min) = timed([fn, double_width], reps)
    res["double_width"] = {"ingest_ms": i_ms, "ingest_ms_min": i_min, "double_width_ms": d_ms, "double_width_ms_min": d_min, "ratio": i_ms / d_ms}
    cases = [("crop_left 0, base + 0", ingest("uyvy422", (0, 2, 0, 0), 0, 2 * W)), ("crop_left 1, base + 0 (spans start 2 bytes off)", ingest("uyvy422", (1, 1, 0, 0), 0, 2 * W)),
             ("crop_left 0, base + 2 bytes", ingest("uyvy422", (0, 2, 0, 0), 2, 2 * W))]
    got = timed([c[1][0] for c in cases], reps)
    res["alignment"] = [{"case": c[0], "ms": g[0], "ms_min": g[1]} for c, g in zip(cases, got)]
    if res_table:
        res["resources"] = res_table
    print(json.dumps(res))
    if notes:
        write_notes(notes, res)


if __name__ == "__main__":
    main()
