"""Python mirror of the reference's operator interface for the binarize path.

`Engine` exposes the VideoToDigital slots a Qt front-end drives (videotodigital.h:137-147) with the same
names and argument meaning - setPCMType, setBinarizationMode, setCheckLineDup, setFineSettings,
setDefaultFineSettings - plus `binarize_frames`, the batch replacement of the doBinarize worker loop.
Everything computes on the GPU through the C-ABI; torch is only used for device memory."""
from __future__ import annotations

import ctypes as C
import os

from . import abi
from .abi import (  # noqa: F401  (what this module defined before abi.py: importable from here as before)
    LINE_DTYPE, STATS_DTYPE, DEINT_LINE_DTYPE, BLOCK_DTYPE, PAIR_DTYPE, AUDIO_PURGE_DTYPE,
    BinPreset, IngestDesc, EncodeDesc, EncodeMarkerlessDesc, DeintSettings, StitchSettings, Pcm1StitchSettings, Pcm16x0StitchSettings, StitchInfo, RunInfo,
    PCM_PCM1, PCM_PCM16X0, PCM_STC007, TYPE_M2, MODE_DRAFT, MODE_FAST, MODE_NORMAL, MODE_INSANE, FLAG_NEW_FILE, FLAG_DOUBLED, FLAG_END_FILE, FRAME_EMPTY,
    DEEMPH_OFF, DEEMPH_AUTO, DEEMPH_FORCE, RESAMPLE_OFF, RESAMPLE_TO_44100, RESAMPLE_DELAY_RIGHT, RESAMPLE_DELAY_LEFT, RESAMPLE_PHASE_HALF,
    PIX_GRAY8, PIX_UYVY422, PIX_YUYV422, PIX_V210, PIX_GRAY10LE, PIX_RGB24, PIX_BGR24, PIX_RGB0, PIX_BGR0, PIX_FORMATS, COLOR_BW, COLOR_R, COLOR_G, COLOR_B,
    INGEST_DOUBLE_OFF, INGEST_DOUBLE_ON, INGEST_DOUBLE_AUTO, ENC_NTSC, ENC_PAL, ENC_14BIT, ENC_16BIT, ENC_TFF, ENC_BFF, ENC_CTRL_COPY_PROHIBITED, ENC_CTRL_EMPHASIS,
    ENC_FMT_PCM1, ENC_FMT_PCM16X0_SI, ENC_FMT_PCM16X0_EI, ENC_ML_EMPHASIS, ENC_ML_RATE_44100, ENC_ML_CODE,
    VIS_STC007_LINES, VIS_PCM1_LINES, VIS_PCM16X0_LINES, VIS_STC007_BLOCKS_NTSC, VIS_STC007_BLOCKS_PAL, VIS_STC007_ASM_NTSC, VIS_STC007_ASM_PAL)

_PKG = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_PKG, "libsdvpcm_hip.so")
_lib = None


def _check_out(t, rec_bytes, device, name):
    """Caller-supplied output tensors: (n, rec_bytes) uint8, contiguous, on the frames' device."""
    import torch
    if not (t.is_cuda and t.device == device and t.dtype == torch.uint8 and t.dim() == 2 and t.shape[1] == rec_bytes and t.is_contiguous()):
        raise ValueError(f"{name} must be a contiguous torch.uint8 CUDA tensor of shape (n, {rec_bytes}) on {device}")


def load_library(path: str | None = None):
    """Loads libsdvpcm_hip.so. Raises (never falls back) when the HIP extension is not built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("SDVPCM_LIB") or _LIB_PATH   # SDVPCM_LIB: alternative builds of the same HIP library (tuning experiments)
    if not os.path.exists(p):
        raise RuntimeError(f"{p} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    lib = abi.bind(C.CDLL(p))
    if path is None:
        _lib = lib
    return lib


class Engine:
    """One decode engine per GPU (per process rank)."""

    def __init__(self, device: int = 0, lib=None):
        # The tensors this class takes are torch's: let torch load and bring up the HIP runtime it ships before the library is loaded
        # and makes its first HIP call - the other way round two runtimes end up in the process and one of them finds no device
        # ("No HIP GPUs are available" / "no HIP device available").
        try:
            import torch
            if torch.cuda.is_available():
                torch.cuda.init()
        except ImportError:
            pass
        self.lib = lib or load_library()
        self.device = device
        self._h = self.lib.sdv_engine_create(device)
        if not self._h:
            raise RuntimeError("sdv_engine_create failed: " + self.lib.sdv_last_error(None).decode())
        self._h = C.c_void_p(self._h)

    def close(self):
        if self._h:
            self.lib.sdv_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise RuntimeError(f"sdvpcm error {rc}: " + self.lib.sdv_last_error(self._h).decode())

    # ---- VideoToDigital slots (videotodigital.h:137-147) ----
    def setPCMType(self, in_pcm: int = PCM_STC007):
        if in_pcm == TYPE_M2:
            self._check(self.lib.sdv_set_pcm_type(self._h, PCM_STC007, 1))
        else:
            self._check(self.lib.sdv_set_pcm_type(self._h, in_pcm, 0))

    def setBinarizationMode(self, in_mode: int = MODE_NORMAL):
        self._check(self.lib.sdv_set_mode(self._h, in_mode))

    def setCheckLineDup(self, flag: bool = True):
        self._check(self.lib.sdv_set_check_line_dup(self._h, int(flag)))

    def getDefaultFineSettings(self) -> BinPreset:
        p = BinPreset()
        self.lib.sdv_default_bin_preset(C.byref(p))
        return p

    def setFineSettings(self, in_set: BinPreset):
        self._check(self.lib.sdv_set_bin_preset(self._h, C.byref(in_set)))

    def setDefaultFineSettings(self):
        self.setFineSettings(self.getDefaultFineSettings())

    def reset_stream(self):
        self._check(self.lib.sdv_reset_stream(self._h))

    def set_frame_flags(self, flags):
        """Per-frame marks for the next frame entry call (binarize_frames / pcm1_binarize_frames / pcm16x0_binarize_frames / decode_frames):
        flags[i] & FRAME_EMPTY = frame i of that call was dropped by the video input (VideoInFFMPEG::insertDummyFrame(false, true))."""
        import numpy as np
        fl = np.ascontiguousarray(flags, dtype=np.uint8)
        self._check(self.lib.sdv_set_frame_flags(self._h, fl.ctypes.data if len(fl) else None, len(fl)))

    def needs_double_width(self, width: int) -> bool:
        return bool(self.lib.sdv_needs_double_width(width))

    def double_width(self, luma, stream=None):
        """The integer 2x width doubler (sdv_double_width): luma (..., width) uint8 CUDA tensor with contiguous rows -> (..., 2 * width)."""
        import torch
        assert luma.is_cuda and luma.dtype == torch.uint8 and luma.stride(-1) == 1 and luma.is_contiguous()
        w = luma.shape[-1]
        rows = luma.numel() // w
        out = torch.empty(luma.shape[:-1] + (2 * w,), dtype=torch.uint8, device=luma.device)
        sptr = C.c_void_p(stream.cuda_stream) if stream is not None else C.c_void_p(torch.cuda.current_stream(luma.device).cuda_stream)
        self._check(self.lib.sdv_double_width(self._h, C.c_void_p(luma.data_ptr()), w, w, rows, C.c_void_p(out.data_ptr()), 2 * w, sptr))
        return out

    def ingest_geometry(self, desc: IngestDesc):
        """sdv_ingest_geometry: (out_width, out_height, doubled, src_row_bytes) of a descriptor; host only."""
        ow, oh, dbl, rb = C.c_int(0), C.c_int(0), C.c_int(0), C.c_size_t(0)
        rc = self.lib.sdv_ingest_geometry(C.byref(desc), C.byref(ow), C.byref(oh), C.byref(dbl), C.byref(rb))
        if rc != 0:
            raise RuntimeError(f"sdvpcm error {rc}: " + self.lib.sdv_last_error(None).decode())
        return ow.value, oh.value, bool(dbl.value), rb.value

    def ingest(self, src, pix_fmt, src_width: int, src_height: int, crop=(0, 0, 0, 0), colors: int = COLOR_BW, double="auto", stream=None):
        """sdv_ingest_frames: captured frames in a packed format -> (luma (n, out_height, out_width) uint8 CUDA tensor, doubled).
        src: uint8 CUDA tensor (n, src_height, row stride in bytes) or (src_height, row stride) whose last dimension is the row in bytes;
        pix_fmt: a PIX_* value or its name; crop: (left, right, top, bottom) in source pixels / rows; double: "off", "on", "auto" or an
        INGEST_DOUBLE_* value.  Pass `doubled` on to the frame entries."""
        import torch
        if not (src.is_cuda and src.dtype == torch.uint8 and src.dim() in (2, 3) and src.stride(-1) == 1):
            raise ValueError("src must be a torch.uint8 CUDA tensor (frames, rows, row bytes) or (rows, row bytes) with contiguous rows")
        if src.dim() == 2:
            src = src.unsqueeze(0)
        if src.shape[1] != src_height:
            raise ValueError(f"src has {src.shape[1]} rows, src_height is {src_height}")
        fmt = PIX_FORMATS[pix_fmt] if isinstance(pix_fmt, str) else int(pix_fmt)
        dbl = {"off": INGEST_DOUBLE_OFF, "on": INGEST_DOUBLE_ON, "auto": INGEST_DOUBLE_AUTO}[double] if isinstance(double, str) else int(double)
        desc = IngestDesc(fmt, colors, dbl, 0, crop[0], crop[1], crop[2], crop[3], src_width, src_height)
        ow, oh, doubled, rb = self.ingest_geometry(desc)
        if src.shape[2] < rb:
            raise ValueError(f"rows of {src.shape[2]} bytes; {src_width} pixels of this format take {rb}")
        n = src.shape[0]
        out = torch.empty((n, oh, ow), dtype=torch.uint8, device=src.device)
        sptr = C.c_void_p(stream.cuda_stream) if stream is not None else C.c_void_p(torch.cuda.current_stream(src.device).cuda_stream)
        self._check(self.lib.sdv_ingest_frames(self._h, C.byref(desc), C.c_void_p(src.data_ptr()), src.stride(1), src.stride(0) if n > 1 else 0, n,
                                               C.c_void_p(out.data_ptr()), ow, oh * ow, sptr))
        return out, doubled

    def encode_geometry(self, desc: EncodeDesc):
        """sdv_encode_geometry: (pairs a frame consumes, lines per field, bytes of a row) of a descriptor; host only."""
        pairs, lines, rb = C.c_size_t(0), C.c_int(0), C.c_size_t(0)
        rc = self.lib.sdv_encode_geometry(C.byref(desc), C.byref(pairs), C.byref(lines), C.byref(rb))
        if rc != 0:
            raise RuntimeError(f"sdvpcm error {rc}: " + self.lib.sdv_last_error(None).decode())
        return pairs.value, lines.value, rb.value

    def encode_frames(self, pcm, n_frames: int, standard="ntsc", bits: int = 14, ctrl_block: bool = False, ctrl_flags: int = 0, bff: bool = False,
                      width: int = 720, height: int = 486, data_start: int = 12, data_stop=None, top_line: int = 0, black: int = 30, white: int = 200,
                      time_code=(0, 0, 0, 0, 0), stream=None, pix_fmt="gray8"):
        """sdv_encode_frames: the next n_frames frames of the tape this engine writes -> (n_frames, height, row_bytes) uint8 CUDA tensor; row_bytes
        is width for pix_fmt "gray8", else the bytes of a packed row (encode_geometry).  pix_fmt: the names ingest takes, or a PIX_* value.
        pcm: torch.int16 CUDA tensor (pairs, 2), interleaved L R; a frame consumes encode_geometry()[0] pairs, pairs that lack are silence (end a
        tape with one frame more from an empty tensor: the interleave delay is played out).  standard: "ntsc" / "pal" or an ENC_* value; bits 14
        or 16; time_code (index, hour, minute, second, field) of the first field after reset_encoder; data_stop defaults to width - 12."""
        import torch
        if not (pcm.is_cuda and pcm.dtype == torch.int16 and pcm.is_contiguous() and (pcm.dim() == 2 and pcm.shape[1] == 2 or pcm.numel() == 0)):
            raise ValueError("pcm must be a contiguous torch.int16 CUDA tensor of shape (pairs, 2)")
        std = {"ntsc": ENC_NTSC, "pal": ENC_PAL}[standard] if isinstance(standard, str) else int(standard)
        if bits not in (14, 16):
            raise ValueError("bits is 14 or 16")
        desc = EncodeDesc(std, ENC_16BIT if bits == 16 else ENC_14BIT, int(bool(ctrl_block)), ctrl_flags, ENC_BFF if bff else ENC_TFF, black, white, 0,
                          time_code[0], time_code[1], time_code[2], time_code[3], time_code[4], (C.c_uint8 * 3)(self._pix_fmt(pix_fmt)), width, height,
                          data_start, width - 12 if data_stop is None else data_stop, top_line)
        row_bytes = self.encode_geometry(desc)[2]
        out = torch.empty((n_frames, height, row_bytes), dtype=torch.uint8, device=pcm.device)
        n_pairs = pcm.numel() // 2
        sptr = C.c_void_p(stream.cuda_stream) if stream is not None else C.c_void_p(torch.cuda.current_stream(pcm.device).cuda_stream)
        self._check(self.lib.sdv_encode_frames(self._h, C.byref(desc), C.c_void_p(pcm.data_ptr()) if n_pairs else None, n_pairs, n_frames,
                                               C.c_void_p(out.data_ptr()), row_bytes, height * row_bytes, sptr))
        return out

    @staticmethod
    def _pix_fmt(pix_fmt):
        """a PIX_* value from its name (as ingest takes it) or itself"""
        if isinstance(pix_fmt, str):
            if pix_fmt not in PIX_FORMATS:
                raise ValueError("pix_fmt is one of " + ", ".join(sorted(PIX_FORMATS)))
            return PIX_FORMATS[pix_fmt]
        return int(pix_fmt) & 0xFF

    def reset_encoder(self):
        """sdv_reset_encoder: the next encode_frames call starts a new tape."""
        self._check(self.lib.sdv_reset_encoder(self._h))

    @staticmethod
    def encode_markerless_desc(fmt="pcm1", bff: bool = False, header_lines: int = 0, emphasis: bool = False, rate_44100: bool = False, code: bool = False,
                               width: int = 720, height: int = 490, data_start: int = 4, data_stop=None, top_line: int = 0, black: int = 30,
                               white: int = 200, pix_fmt="gray8") -> EncodeMarkerlessDesc:
        """The descriptor of encode_markerless_frames' keywords.  fmt: "pcm1" / "pcm16x0_si" / "pcm16x0_ei" or an ENC_FMT_* value; pix_fmt: the
        names ingest takes, or a PIX_* value."""
        formats = {"pcm1": ENC_FMT_PCM1, "pcm16x0_si": ENC_FMT_PCM16X0_SI, "pcm16x0_ei": ENC_FMT_PCM16X0_EI}
        if isinstance(fmt, str) and fmt not in formats:
            raise ValueError("fmt is one of " + ", ".join(sorted(formats)))
        flags = (ENC_ML_EMPHASIS if emphasis else 0) | (ENC_ML_RATE_44100 if rate_44100 else 0) | (ENC_ML_CODE if code else 0)
        return EncodeMarkerlessDesc(formats[fmt] if isinstance(fmt, str) else int(fmt), ENC_BFF if bff else ENC_TFF, black, white, header_lines, flags,
                                    (C.c_uint8 * 2)(Engine._pix_fmt(pix_fmt)), width, height, data_start, width - 4 if data_stop is None else data_stop, top_line)

    def encode_markerless_geometry(self, desc: EncodeMarkerlessDesc):
        """sdv_encode_markerless_geometry: (pairs a frame consumes, lines per field, bytes of a row) of a descriptor; host only."""
        pairs, lines, rb = C.c_size_t(0), C.c_int(0), C.c_size_t(0)
        rc = self.lib.sdv_encode_markerless_geometry(C.byref(desc), C.byref(pairs), C.byref(lines), C.byref(rb))
        if rc != 0:
            raise RuntimeError(f"sdvpcm error {rc}: " + self.lib.sdv_last_error(None).decode())
        return pairs.value, lines.value, rb.value

    def encode_markerless_frames(self, pcm, n_frames: int, fmt="pcm1", stream=None, **kw):
        """sdv_encode_markerless_frames: n_frames frames of a PCM-1 or PCM-16x0 tape -> (n_frames, height, row_bytes) uint8 CUDA tensor; row_bytes
        is width unless the keyword pix_fmt asks for a packed format.
        pcm: torch.int16 CUDA tensor (pairs, 2), interleaved L R; a frame takes 1470 pairs, pairs that lack are silence.  There is no state: the next
        call goes on with pcm[1470 * n_frames:].  The keywords are those of encode_markerless_desc; data_stop defaults to width - 4.  PCM-1 wants
        header_lines = 1 (and height 492) for a tape the decoder reads without a forced-bad first line."""
        import torch
        if not (pcm.is_cuda and pcm.dtype == torch.int16 and pcm.is_contiguous() and (pcm.dim() == 2 and pcm.shape[1] == 2 or pcm.numel() == 0)):
            raise ValueError("pcm must be a contiguous torch.int16 CUDA tensor of shape (pairs, 2)")
        desc = self.encode_markerless_desc(fmt, **kw)
        row_bytes = self.encode_markerless_geometry(desc)[2]
        out = torch.empty((n_frames, desc.height, row_bytes), dtype=torch.uint8, device=pcm.device)
        n_pairs = pcm.numel() // 2
        sptr = C.c_void_p(stream.cuda_stream) if stream is not None else C.c_void_p(torch.cuda.current_stream(pcm.device).cuda_stream)
        self._check(self.lib.sdv_encode_markerless_frames(self._h, C.byref(desc), C.c_void_p(pcm.data_ptr()) if n_pairs else None, n_pairs, n_frames,
                                                          C.c_void_p(out.data_ptr()), row_bytes, desc.height * row_bytes, sptr))
        return out

    # ---- ahead of the encoders: pre-emphasis and 44 100 -> 44 056 Hz on (pairs, 2) int16 PCM: beyond the reference ----------------------
    @staticmethod
    def _check_pcm(t, name):
        import torch
        if not (t.is_cuda and t.dtype == torch.int16 and t.is_contiguous() and t.dim() == 2 and t.shape[1] == 2):
            raise ValueError(name + " must be a contiguous torch.int16 CUDA tensor of shape (pairs, 2)")

    def preemphasis_coeffs(self, rate: int):
        """(c0, c1, c2) of the pre-emphasis network at a rate (44056, anything else reads 44100)."""
        c = (C.c_double * 3)()
        self.lib.sdv_preemphasis_coeffs(int(rate), c)
        return tuple(c)

    def reset_preemphasis(self):
        """The filter forgets the stream it was on (the next pair starts it, its word stays); the counter of clipped samples is 0."""
        self._check(self.lib.sdv_reset_preemphasis(self._h))

    def pcm_preemphasis(self, pcm, sample_rate: int, out=None, stream=None):
        """The 15/50 us network, the inverse of audio_deemphasis, over one burst of a PCM stream: (n, 2) int16 -> (n, 2) int16 on the device,
        asynchronous on the stream.  sample_rate: the tape's, 44056 or 44100.  out: a buffer that does not overlap `pcm`; the filter state and
        the counter of clipped samples stay in the engine from call to call."""
        import torch
        self._check_pcm(pcm, "pcm")
        n = pcm.shape[0]
        if out is None:
            out = torch.empty((n, 2), dtype=torch.int16, device=pcm.device)
        self._check_pcm(out, "out")
        if out.shape[0] < n:
            raise ValueError("out holds fewer pairs than pcm")
        sptr = C.c_void_p(stream.cuda_stream) if stream is not None else C.c_void_p(torch.cuda.current_stream(pcm.device).cuda_stream)
        self._check(self.lib.sdv_pcm_preemphasis(self._h, C.c_void_p(pcm.data_ptr()) if n else None, n, int(sample_rate),
                                                 C.c_void_p(out.data_ptr()) if n else None, sptr))
        return out[:n]

    def preemphasis_clipped(self, stream=None) -> int:
        """Samples the pre-emphasis clipped since the engine was made or reset_preemphasis, both channels summed; waits for the stream."""
        import torch
        sptr = C.c_void_p(stream.cuda_stream) if stream is not None else C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        n = C.c_uint64(0)
        self._check(self.lib.sdv_pcm_preemphasis_clipped(self._h, sptr, C.byref(n)))
        return int(n.value)

    def pcm_resample_taps(self, phase: int):
        """The 128 taps of a phase (0 .. 999) of pcm_resample, as a tuple of floats."""
        c = (C.c_double * 128)()
        self.lib.sdv_pcm_resample_taps(int(phase), c)
        return tuple(c)

    def reset_pcm_resample(self):
        """No open stream, nothing pending."""
        self._check(self.lib.sdv_reset_pcm_resample(self._h))

    def pcm_resample_pending(self) -> int:
        return int(self.lib.sdv_pcm_resample_pending(self._h))

    def pcm_resample(self, pcm, flush=False, out=None, stream=None):
        """One burst of a 44 100 Hz PCM stream through the 1000 / 1001 resampler: (n, 2) int16 -> (n_out, 2) int16 at 44 056 Hz on the device,
        asynchronous on the stream.  Without flush the last 64 pairs wait in the engine for the next call; flush closes the stream.  out: a buffer
        of at least sdv_pcm_resample_room pairs that does not overlap `pcm`."""
        import torch
        self._check_pcm(pcm, "pcm")
        n = pcm.shape[0]
        room = int(self.lib.sdv_pcm_resample_room(self._h, n))
        if out is None:
            out = torch.empty((room, 2), dtype=torch.int16, device=pcm.device)
        self._check_pcm(out, "out")
        sptr = C.c_void_p(stream.cuda_stream) if stream is not None else C.c_void_p(torch.cuda.current_stream(pcm.device).cuda_stream)
        n_out = C.c_size_t(0)
        self._check(self.lib.sdv_pcm_resample(self._h, C.c_void_p(pcm.data_ptr()) if n else None, n, 1 if flush else 0,
                                              C.c_void_p(out.data_ptr()) if out.shape[0] else None, out.shape[0], C.byref(n_out), sptr))
        return out[:n_out.value]

    # ---- visualiser feed (RenderPCM's canvas of binarized lines) ----
    def vis_canvas_size(self, kind: int):
        w, h = C.c_uint32(0), C.c_uint32(0)
        self._check(self.lib.sdv_vis_canvas_size(kind, C.byref(w), C.byref(h)))
        return w.value, h.value

    def vis_reset(self, kind: int, stream=None):
        import torch
        sptr = C.c_void_p(stream.cuda_stream) if stream is not None else C.c_void_p(torch.cuda.current_stream().cuda_stream)
        self._check(self.lib.sdv_vis_reset(self._h, kind, sptr))

    def vis_render_lines(self, kind: int, recs, n_frames: int, stream=None):
        """sdv_vis_render_lines: `recs` = (n, record size) uint8 CUDA tensor of the kind's line records holding `n_frames` whole frames
        -> (n_frames, height, width) int32 CUDA tensor of 32-bit pixels (view it as uint32 on the host)."""
        import torch
        assert recs.is_cuda and recs.dtype == torch.uint8 and recs.is_contiguous()
        w, h = self.vis_canvas_size(kind)
        out = torch.empty((max(n_frames, 1), h, w), dtype=torch.int32, device=recs.device)
        got = C.c_size_t(0)
        sptr = C.c_void_p(stream.cuda_stream) if stream is not None else C.c_void_p(torch.cuda.current_stream(recs.device).cuda_stream)
        self._check(self.lib.sdv_vis_render_lines(self._h, kind, C.c_void_p(recs.data_ptr()), recs.shape[0], C.c_void_p(out.data_ptr()), n_frames,
                                                  C.byref(got), sptr))
        return out[:got.value]

    def set_stitch_block_output(self, blocks):
        """sdv_set_stitch_block_output: `blocks` = (cap, 72) uint8 CUDA tensor that the following stitch_frames calls fill with their data
        blocks (None: off).  The tensor must stay alive while it is set."""
        self._block_out = blocks
        if blocks is None:
            self._check(self.lib.sdv_set_stitch_block_output(self._h, None, 0))
        else:
            assert blocks.is_cuda and blocks.is_contiguous() and blocks.shape[1] == 72
            self._check(self.lib.sdv_set_stitch_block_output(self._h, C.c_void_p(blocks.data_ptr()), blocks.shape[0]))

    def stitch_block_count(self) -> int:
        return int(self.lib.sdv_stitch_block_count(self._h))

    def set_stitch_line_output(self, lines):
        """sdv_set_stitch_line_output: `lines` = (cap, 32) uint8 CUDA tensor that the following stitch_frames calls fill with the assembled lines
        they hand to the visualiser (None: off).  The tensor must stay alive while it is set."""
        self._line_out = lines
        if lines is None:
            self._check(self.lib.sdv_set_stitch_line_output(self._h, None, 0))
        else:
            assert lines.is_cuda and lines.is_contiguous() and lines.shape[1] == 32
            self._check(self.lib.sdv_set_stitch_line_output(self._h, C.c_void_p(lines.data_ptr()), lines.shape[0]))

    def stitch_line_count(self) -> int:
        return int(self.lib.sdv_stitch_line_count(self._h))

    def stitch_line_counts(self):
        """Lines per stitcher turn of the last stitch_frames call (numpy uint32)."""
        import numpy as np
        n = int(self.lib.sdv_stitch_line_counts(self._h, None, 0))
        out = np.zeros(max(n, 1), dtype=np.uint32)
        self.lib.sdv_stitch_line_counts(self._h, out.ctypes.data, n)
        return out[:n]

    def vis_render_asm_lines(self, kind: int, lines, frame_lines, stream=None):
        """sdv_vis_render_asm_lines: `lines` = (n, 32) uint8 CUDA tensor of sdv_asm_line_rec, frame_lines = lines per frame (host sequence)
        -> (n_frames, height, width) int32 CUDA tensor."""
        import numpy as np
        import torch
        assert lines.is_cuda and lines.dtype == torch.uint8 and lines.is_contiguous()
        per = np.ascontiguousarray(np.asarray(frame_lines, dtype=np.uint32))
        w, h = self.vis_canvas_size(kind)
        out = torch.empty((max(len(per), 1), h, w), dtype=torch.int32, device=lines.device)
        sptr = C.c_void_p(stream.cuda_stream) if stream is not None else C.c_void_p(torch.cuda.current_stream(lines.device).cuda_stream)
        self._check(self.lib.sdv_vis_render_asm_lines(self._h, kind, C.c_void_p(lines.data_ptr()), lines.shape[0], per.ctypes.data, len(per),
                                                      C.c_void_p(out.data_ptr()), len(per), sptr))
        return out[:len(per)]

    def vis_render_blocks(self, kind: int, blocks, frame_blocks, stream=None):
        """sdv_vis_render_blocks: `blocks` = (n, 72) uint8 CUDA tensor of sdv_block_rec, frame_blocks = blocks per frame (host sequence)
        -> (n_frames, height, width) int32 CUDA tensor."""
        import numpy as np
        import torch
        assert blocks.is_cuda and blocks.dtype == torch.uint8 and blocks.is_contiguous()
        per = np.ascontiguousarray(np.asarray(frame_blocks, dtype=np.uint32))
        w, h = self.vis_canvas_size(kind)
        out = torch.empty((max(len(per), 1), h, w), dtype=torch.int32, device=blocks.device)
        sptr = C.c_void_p(stream.cuda_stream) if stream is not None else C.c_void_p(torch.cuda.current_stream(blocks.device).cuda_stream)
        self._check(self.lib.sdv_vis_render_blocks(self._h, kind, C.c_void_p(blocks.data_ptr()), blocks.shape[0], per.ctypes.data, len(per),
                                                   C.c_void_p(out.data_ptr()), len(per), sptr))
        return out[:len(per)]

    # ---- stream state as bytes (checkpoints, hand-over between the GPUs of a sharded stream) ----
    def get_chain_state(self) -> bytes:
        buf = C.create_string_buffer(120)
        self._check(self.lib.sdv_get_chain_state(self._h, buf))
        return buf.raw

    def set_chain_state(self, state: bytes):
        assert len(state) == 120
        self._check(self.lib.sdv_set_chain_state(self._h, C.create_string_buffer(state, 120)))

    def get_stitch_state(self) -> bytes:
        n = self.lib.sdv_stitch_state_size()
        buf = C.create_string_buffer(n)
        self._check(self.lib.sdv_get_stitch_state(self._h, buf, n))
        return buf.raw

    def set_stitch_state(self, state: bytes):
        self._check(self.lib.sdv_set_stitch_state(self._h, C.create_string_buffer(state, len(state)), len(state)))

    def saturate_stitch_stats(self):
        self._check(self.lib.sdv_saturate_stitch_stats(self._h))

    def get_pcm16x0_chain_state(self) -> bytes:
        n = self.lib.sdv_pcm16x0_chain_state_size()
        buf = C.create_string_buffer(n)
        self._check(self.lib.sdv_get_pcm16x0_chain_state(self._h, buf, n))
        return buf.raw

    def set_pcm16x0_chain_state(self, state: bytes):
        self._check(self.lib.sdv_set_pcm16x0_chain_state(self._h, C.create_string_buffer(state, len(state)), len(state)))

    def get_pcm16x0_stitch_state(self) -> bytes:
        n = self.lib.sdv_pcm16x0_stitch_state_size()
        buf = C.create_string_buffer(n)
        self._check(self.lib.sdv_get_pcm16x0_stitch_state(self._h, buf, n))
        return buf.raw

    def set_pcm16x0_stitch_state(self, state: bytes):
        self._check(self.lib.sdv_set_pcm16x0_stitch_state(self._h, C.create_string_buffer(state, len(state)), len(state)))

    def saturate_pcm16x0_stitch_stats(self):
        self._check(self.lib.sdv_saturate_pcm16x0_stitch_stats(self._h))

    def set_profiling(self, on: bool = True):
        self._check(self.lib.sdv_set_profiling(self._h, int(on)))

    def run_info(self) -> RunInfo:
        info = RunInfo()
        self.lib.sdv_get_run_info(self._h, C.byref(info))
        return info

    # ---- STC007Deinterleaver (stc007deinterleaver.h:163-176) ----
    def default_deint_settings(self) -> DeintSettings:
        st = DeintSettings()
        self.lib.sdv_default_deint_settings(C.byref(st))
        return st

    def deinterleave_blocks(self, lines, settings: DeintSettings, n_blocks: int | None = None, out=None, stream=None):
        """processBlock(line_shift) for line_shift = 0..n_blocks-1 over `lines` (torch.uint8 CUDA tensor (n_lines, 24)).
        Returns torch.uint8 CUDA tensor (n_blocks, 72) of sdv_block_rec."""
        import torch
        assert lines.is_cuda and lines.dtype == torch.uint8 and lines.dim() == 2 and lines.shape[1] == 24 and lines.is_contiguous()
        n_lines = lines.shape[0]
        if n_blocks is None:
            n_blocks = max(0, n_lines - 112)
        if out is None:
            out = torch.empty((n_blocks, 72), dtype=torch.uint8, device=lines.device)
        sptr = C.c_void_p(stream.cuda_stream) if stream is not None else C.c_void_p(torch.cuda.current_stream(lines.device).cuda_stream)
        self._check(self.lib.sdv_deinterleave_blocks(self._h, C.c_void_p(lines.data_ptr()), n_lines, C.byref(settings),
                                                     C.c_void_p(out.data_ptr()), n_blocks, sptr))
        return out

    # ---- STC007DataStitcher (stc007datastitcher.h:331-350) ----
    def default_stitch_settings(self) -> StitchSettings:
        st = StitchSettings()
        self.lib.sdv_default_stitch_settings(C.byref(st))
        return st

    def set_stitch_settings(self, st: StitchSettings):
        self._check(self.lib.sdv_set_stitch_settings(self._h, C.byref(st)))

    def reset_stitcher(self):
        self._check(self.lib.sdv_reset_stitcher(self._h))

    def stitch_info(self) -> StitchInfo:
        info = StitchInfo()
        self.lib.sdv_get_stitch_info(self._h, C.byref(info))
        return info

    def stitch_frames(self, lines, out_pairs=None, out_frames=None, stream=None):
        """doFrameReassemble over a span of the binarized line stream: `lines` is a torch.uint8 CUDA tensor (n_records, 48)
        (what binarize_frames returns).  Returns (pairs, frames): torch.uint8 CUDA tensors (n_pairs, 12) of sdv_sample_pair
        and (n_frames, 64) of sdv_frame_asm - views of out_pairs / out_frames when those are given."""
        import torch
        assert lines.is_cuda and lines.dtype == torch.uint8 and lines.dim() == 2 and lines.shape[1] == 48 and lines.is_contiguous()
        n = lines.shape[0]
        if out_pairs is None:
            out_pairs = torch.empty((n * 13 // 4 + 8192, 12), dtype=torch.uint8, device=lines.device)   # 3 pairs per assembled line + padding
        if out_frames is None:
            out_frames = torch.empty((n // 8 + 64, 64), dtype=torch.uint8, device=lines.device)
        sptr = C.c_void_p(stream.cuda_stream) if stream is not None else C.c_void_p(torch.cuda.current_stream(lines.device).cuda_stream)
        npairs, nframes = C.c_size_t(0), C.c_size_t(0)
        rc = self.lib.sdv_stitch_frames(self._h, C.c_void_p(lines.data_ptr()), n, C.c_void_p(out_pairs.data_ptr()), out_pairs.shape[0],
                                        C.byref(npairs), C.c_void_p(out_frames.data_ptr()), out_frames.shape[0], C.byref(nframes), sptr)
        self._check(rc)
        return out_pairs[:npairs.value], out_frames[:nframes.value]

    # ---- PCM-1 back half (PCM1DataStitcher) ----
    def default_pcm1_stitch_settings(self) -> Pcm1StitchSettings:
        st = Pcm1StitchSettings()
        self.lib.sdv_default_pcm1_stitch_settings(C.byref(st))
        return st

    def set_pcm1_stitch_settings(self, st: Pcm1StitchSettings):
        self._check(self.lib.sdv_set_pcm1_stitch_settings(self._h, C.byref(st)))

    def pcm1_stitch_frames(self, lines, out_pairs=None, out_frames=None, stream=None):
        """PCM1DataStitcher::doFrameReassemble over a span of the PCM-1 line stream: `lines` is a torch.uint8 CUDA tensor
        (n_records, 32) of sdv_pcm1_line_rec.  Returns (pairs, frames): torch.uint8 CUDA tensors (n_pairs, 12) of sdv_sample_pair
        and (n_frames, 52) of sdv_frame_asm_pcm1."""
        import torch
        assert lines.is_cuda and lines.dtype == torch.uint8 and lines.dim() == 2 and lines.shape[1] == 32 and lines.is_contiguous()
        n = lines.shape[0]
        own_pairs, own_frames = out_pairs is None, out_frames is None
        if out_pairs is None:
            out_pairs = torch.empty((n * 3 + 4096, 12), dtype=torch.uint8, device=lines.device)     # 3 pairs per line + padding lines
        if out_frames is None:
            out_frames = torch.empty((n // 64 + 64, 52), dtype=torch.uint8, device=lines.device)
        sptr = C.c_void_p(stream.cuda_stream) if stream is not None else C.c_void_p(torch.cuda.current_stream(lines.device).cuda_stream)
        npairs, nframes = C.c_size_t(0), C.c_size_t(0)
        for attempt in (0, 1):
            rc = self.lib.sdv_pcm1_stitch_frames(self._h, C.c_void_p(lines.data_ptr()), n, C.c_void_p(out_pairs.data_ptr()), out_pairs.shape[0],
                                                 C.byref(npairs), C.c_void_p(out_frames.data_ptr()), out_frames.shape[0], C.byref(nframes), sptr)
            # buffers of our own guess were too small (a frame that lost most of its lines still decodes to 1470 pairs; lines that waited in the engine
            # complete frames): the refused call took nothing and reported the sizes - once more with those
            if rc == -1 and attempt == 0 and (npairs.value > out_pairs.shape[0] or nframes.value > out_frames.shape[0]) and \
                    (own_pairs or npairs.value <= out_pairs.shape[0]) and (own_frames or nframes.value <= out_frames.shape[0]):
                if own_pairs and npairs.value > out_pairs.shape[0]:
                    out_pairs = torch.empty((npairs.value, 12), dtype=torch.uint8, device=lines.device)
                if own_frames and nframes.value > out_frames.shape[0]:
                    out_frames = torch.empty((nframes.value, 52), dtype=torch.uint8, device=lines.device)
                continue
            break
        self._check(rc)
        return out_pairs[:npairs.value], out_frames[:nframes.value]

    def set_pcm1_stitch_block_output(self, blocks):
        """sdv_set_pcm1_stitch_block_output: `blocks` = (cap, 576) uint8 CUDA tensor the following pcm1_stitch_frames calls fill with their
        PCM1DataBlocks, 16 per frame (None: off).  The tensor must stay alive while it is set."""
        self._p1_block_out = blocks
        if blocks is None:
            self._check(self.lib.sdv_set_pcm1_stitch_block_output(self._h, None, 0))
        else:
            assert blocks.is_cuda and blocks.is_contiguous() and blocks.shape[1] == 576
            self._check(self.lib.sdv_set_pcm1_stitch_block_output(self._h, C.c_void_p(blocks.data_ptr()), blocks.shape[0]))

    def pcm1_stitch_block_count(self) -> int:
        return int(self.lib.sdv_pcm1_stitch_block_count(self._h))

    def set_pcm1_stitch_line_output(self, lines):
        """sdv_set_pcm1_stitch_line_output: `lines` = (cap, 16) uint8 CUDA tensor for the sub-lines of the stitcher's queue, 1470 per frame."""
        self._p1_line_out = lines
        if lines is None:
            self._check(self.lib.sdv_set_pcm1_stitch_line_output(self._h, None, 0))
        else:
            assert lines.is_cuda and lines.is_contiguous() and lines.shape[1] == 16
            self._check(self.lib.sdv_set_pcm1_stitch_line_output(self._h, C.c_void_p(lines.data_ptr()), lines.shape[0]))

    def pcm1_stitch_line_count(self) -> int:
        return int(self.lib.sdv_pcm1_stitch_line_count(self._h))

    def set_pcm16x0_stitch_block_output(self, blocks):
        """sdv_set_pcm16x0_stitch_block_output: `blocks` = (cap, 32) uint8 CUDA tensor the following pcm16x0_stitch_frames calls fill with their
        PCM16X0DataBlocks (None: off).  The tensor must stay alive while it is set."""
        self._p16_block_out = blocks
        if blocks is None:
            self._check(self.lib.sdv_set_pcm16x0_stitch_block_output(self._h, None, 0))
        else:
            assert blocks.is_cuda and blocks.is_contiguous() and blocks.shape[1] == 32
            self._check(self.lib.sdv_set_pcm16x0_stitch_block_output(self._h, C.c_void_p(blocks.data_ptr()), blocks.shape[0]))

    def pcm16x0_stitch_block_count(self) -> int:
        return int(self.lib.sdv_pcm16x0_stitch_block_count(self._h))

    def set_pcm16x0_stitch_line_output(self, lines):
        """sdv_set_pcm16x0_stitch_line_output: `lines` = (cap, 36) uint8 CUDA tensor the following pcm16x0_stitch_frames calls fill with the assembled
        sub-lines of their frames as sdv_pcm16x0_bin_rec, an END_FRAME record behind every frame's (None: off) - what vis_render_lines(PCM16X0_LINES)
        draws as the reference's re-assembled window.  The tensor must stay alive while it is set."""
        self._p16_line_out = lines
        if lines is None:
            self._check(self.lib.sdv_set_pcm16x0_stitch_line_output(self._h, None, 0))
        else:
            assert lines.is_cuda and lines.is_contiguous() and lines.shape[1] == 36
            self._check(self.lib.sdv_set_pcm16x0_stitch_line_output(self._h, C.c_void_p(lines.data_ptr()), lines.shape[0]))

    def pcm16x0_stitch_line_count(self) -> int:
        return int(self.lib.sdv_pcm16x0_stitch_line_count(self._h))

    def pcm1_bin_to_line_recs(self, bin_recs, out=None, stream=None):
        """The records pcm1_binarize_frames returns ((n, 40) sdv_pcm1_bin_rec) as the records pcm1_stitch_frames takes ((n, 32) sdv_pcm1_line_rec)."""
        import torch
        _check_out(bin_recs, 40, bin_recs.device, "bin_recs")
        n = bin_recs.shape[0]
        if out is None:
            out = torch.empty((n, 32), dtype=torch.uint8, device=bin_recs.device)
        _check_out(out, 32, bin_recs.device, "out")
        sptr = C.c_void_p(stream.cuda_stream) if stream is not None else C.c_void_p(torch.cuda.current_stream(bin_recs.device).cuda_stream)
        self._check(self.lib.sdv_pcm1_bin_to_line_recs(self._h, C.c_void_p(bin_recs.data_ptr()), n, C.c_void_p(out.data_ptr()), sptr))
        return out[:n]

    def default_pcm16x0_stitch_settings(self) -> Pcm16x0StitchSettings:
        st = Pcm16x0StitchSettings()
        self.lib.sdv_default_pcm16x0_stitch_settings(C.byref(st))
        return st

    def set_pcm16x0_stitch_settings(self, st: Pcm16x0StitchSettings):
        """Applies the settings and starts a fresh PCM16X0DataStitcher (histories and waiting sub-lines are dropped)."""
        self._check(self.lib.sdv_set_pcm16x0_stitch_settings(self._h, C.byref(st)))

    def pcm16x0_stitch_frames(self, lines, out_pairs=None, out_frames=None, stream=None):
        """PCM16X0DataStitcher::doFrameReassemble over a span of the PCM-16x0 sub-line stream: `lines` is a torch.uint8 CUDA tensor
        (n_records, 36) of sdv_pcm16x0_bin_rec (what pcm16x0_binarize_frames returns).  Returns (pairs, frames): torch.uint8 CUDA tensors
        (n_pairs, 12) of sdv_sample_pair and (n_frames, 56) of sdv_frame_asm_pcm16x0."""
        import torch
        assert lines.is_cuda and lines.dtype == torch.uint8 and lines.dim() == 2 and lines.shape[1] == 36 and lines.is_contiguous()
        n = lines.shape[0]
        own_pairs, own_frames = out_pairs is None, out_frames is None
        if out_pairs is None:
            out_pairs = torch.empty((n + n // 8 + 4096, 12), dtype=torch.uint8, device=lines.device)     # a pair per sub-line + padding
        if out_frames is None:
            out_frames = torch.empty((n // 64 + 64, 56), dtype=torch.uint8, device=lines.device)
        _check_out(out_pairs, 12, lines.device, "out_pairs")
        _check_out(out_frames, 56, lines.device, "out_frames")
        sptr = C.c_void_p(stream.cuda_stream) if stream is not None else C.c_void_p(torch.cuda.current_stream(lines.device).cuda_stream)
        npairs, nframes = C.c_size_t(0), C.c_size_t(0)
        for attempt in (0, 1):
            rc = self.lib.sdv_pcm16x0_stitch_frames(self._h, C.c_void_p(lines.data_ptr()), n, C.c_void_p(out_pairs.data_ptr()), out_pairs.shape[0],
                                                    C.byref(npairs), C.c_void_p(out_frames.data_ptr()), out_frames.shape[0], C.byref(nframes), sptr)
            # buffers of our own guess were too small (short fields still decode to 1470 pairs a frame): the refused call took
            # nothing and reported the sizes - once more with those
            if rc == -1 and attempt == 0 and (npairs.value > out_pairs.shape[0] or nframes.value > out_frames.shape[0]) and \
                    (own_pairs or npairs.value <= out_pairs.shape[0]) and (own_frames or nframes.value <= out_frames.shape[0]):
                if npairs.value > out_pairs.shape[0]:
                    out_pairs = torch.empty((npairs.value, 12), dtype=torch.uint8, device=lines.device)
                if nframes.value > out_frames.shape[0]:
                    out_frames = torch.empty((nframes.value, 56), dtype=torch.uint8, device=lines.device)
                continue
            break
        self._check(rc)
        return out_pairs[:npairs.value], out_frames[:nframes.value]

    def binarize_lines(self, luma, presets=None, frame_number: int = 1, first_line: int = 1, line_step: int = 1, doubled: bool = False, out_lines=None, stream=None):
        """Binarizer::processLine with an STC007Line output for every row of `luma` (torch.uint8 CUDA tensor (n_lines, width), rows contiguous) in one
        call.  `presets`: None or a torch.uint8 CUDA tensor (n_lines, 10) of sdv_bin_state - what the caller's Binarizer had been given before each line.
        Returns a torch.uint8 CUDA tensor (n_lines, 48) of sdv_line_rec, the lines as processLine leaves them (no VideoToDigital bookkeeping)."""
        import torch
        assert luma.is_cuda and luma.dtype == torch.uint8 and luma.dim() == 2 and luma.stride(1) == 1
        n, w = luma.shape
        if presets is not None:
            assert presets.is_cuda and presets.dtype == torch.uint8 and presets.shape == (n, 10) and presets.is_contiguous()
        if out_lines is None:
            out_lines = torch.empty((n, 48), dtype=torch.uint8, device=luma.device)
        _check_out(out_lines, 48, luma.device, "out_lines")
        sptr = C.c_void_p(stream.cuda_stream) if stream is not None else C.c_void_p(torch.cuda.current_stream(luma.device).cuda_stream)
        rc = self.lib.sdv_binarize_lines(self._h, C.c_void_p(luma.data_ptr()), luma.stride(0), w, n,
                                         None if presets is None else C.c_void_p(presets.data_ptr()), frame_number, first_line, line_step,
                                         FLAG_DOUBLED if doubled else 0, C.c_void_p(out_lines.data_ptr()), out_lines.shape[0], sptr)
        self._check(rc)
        return out_lines[:n]

    def pcm1_binarize_lines(self, luma, presets=None, frame_number: int = 1, first_line: int = 1, line_step: int = 1, doubled: bool = False,
                            coord_search: bool = True, out_lines=None, stream=None):
        """Binarizer::processLine with a PCM1Line output for every row of `luma` (torch.uint8 CUDA tensor (n_lines, width), rows
        contiguous) in one launch.  `presets`: None or a torch.uint8 CUDA tensor (n_lines, 10) of sdv_bin_state - what the caller's
        Binarizer had been given before each line.  Returns a torch.uint8 CUDA tensor (n_lines, 40) of sdv_pcm1_bin_rec."""
        import torch
        assert luma.is_cuda and luma.dtype == torch.uint8 and luma.dim() == 2 and luma.stride(1) == 1
        n, w = luma.shape
        if presets is not None:
            assert presets.is_cuda and presets.dtype == torch.uint8 and presets.shape == (n, 10) and presets.is_contiguous()
        if out_lines is None:
            out_lines = torch.empty((n, 40), dtype=torch.uint8, device=luma.device)
        _check_out(out_lines, 40, luma.device, "out_lines")
        sptr = C.c_void_p(stream.cuda_stream) if stream is not None else C.c_void_p(torch.cuda.current_stream(luma.device).cuda_stream)
        rc = self.lib.sdv_pcm1_binarize_lines(self._h, C.c_void_p(luma.data_ptr()), luma.stride(0), w, n,
                                              None if presets is None else C.c_void_p(presets.data_ptr()), frame_number, first_line, line_step,
                                              FLAG_DOUBLED if doubled else 0, 1 if coord_search else 0, C.c_void_p(out_lines.data_ptr()),
                                              out_lines.shape[0], sptr)
        self._check(rc)
        return out_lines[:n]

    def pcm16x0_binarize_lines(self, luma, presets=None, frame_number: int = 1, first_line: int = 1, line_step: int = 1, doubled: bool = False,
                               coord_search: bool = True, out_lines=None, with_scan_done: bool = False, stream=None):
        """Binarizer::processLine with a PCM16X0SubLine output, the three passes over every row of `luma` (torch.uint8 CUDA tensor
        (n_lines, width), rows contiguous) in one launch.  `presets`: None or a torch.uint8 CUDA tensor (3 * n_lines, 10) of sdv_bin_state -
        what the caller's Binarizer had been given before each pass.  Returns a torch.uint8 CUDA tensor (3 * n_lines, 36) of
        sdv_pcm16x0_bin_rec (and, with_scan_done, a uint8 tensor of VideoLine::scan_done behind each pass)."""
        import torch
        assert luma.is_cuda and luma.dtype == torch.uint8 and luma.dim() == 2 and luma.stride(1) == 1
        n, w = luma.shape
        if presets is not None:
            assert presets.is_cuda and presets.dtype == torch.uint8 and presets.shape == (3 * n, 10) and presets.is_contiguous()
        if out_lines is None:
            out_lines = torch.empty((3 * n, 36), dtype=torch.uint8, device=luma.device)
        _check_out(out_lines, 36, luma.device, "out_lines")
        scans = torch.zeros((3 * n,), dtype=torch.uint8, device=luma.device) if with_scan_done else None
        sptr = C.c_void_p(stream.cuda_stream) if stream is not None else C.c_void_p(torch.cuda.current_stream(luma.device).cuda_stream)
        rc = self.lib.sdv_pcm16x0_binarize_lines(self._h, C.c_void_p(luma.data_ptr()), luma.stride(0), w, n,
                                                 None if presets is None else C.c_void_p(presets.data_ptr()), frame_number, first_line, line_step,
                                                 FLAG_DOUBLED if doubled else 0, 1 if coord_search else 0, C.c_void_p(out_lines.data_ptr()),
                                                 out_lines.shape[0], None if scans is None else C.c_void_p(scans.data_ptr()), sptr)
        self._check(rc)
        return (out_lines[:3 * n], scans) if with_scan_done else out_lines[:3 * n]

    def pcm1_binarize_frames(self, luma, first_frame_no: int = 1, new_file: bool = False, doubled: bool = False,
                             out_lines=None, out_stats=None, stream=None, end_file: bool = False):
        """VideoToDigital::doBinarize with setPCMType(TYPE_PCM1) over whole frames: luma is a torch.uint8 CUDA tensor
        (n_frames, height, width).  Returns (lines, stats): torch.uint8 CUDA tensors (n_records, 40) of sdv_pcm1_bin_rec and
        (n_frames, 32) of sdv_frame_stats; record order and counts as for binarize_frames."""
        import torch
        assert luma.is_cuda and luma.dtype == torch.uint8 and luma.dim() == 3 and luma.stride(2) == 1
        n, h, w = luma.shape
        nrec = n * (h + 3) + (1 if new_file else 0) + (h + 4 if end_file else 0)
        nst = n + (1 if end_file else 0)
        if out_lines is None:
            out_lines = torch.empty((nrec, 40), dtype=torch.uint8, device=luma.device)
        if out_stats is None:
            out_stats = torch.empty((nst, 32), dtype=torch.uint8, device=luma.device)
        _check_out(out_lines, 40, luma.device, "out_lines")
        _check_out(out_stats, 32, luma.device, "out_stats")
        flags = (FLAG_NEW_FILE if new_file else 0) | (FLAG_DOUBLED if doubled else 0) | (FLAG_END_FILE if end_file else 0)
        sptr = C.c_void_p(stream.cuda_stream) if stream is not None else C.c_void_p(torch.cuda.current_stream(luma.device).cuda_stream)
        rc = self.lib.sdv_pcm1_binarize_frames(self._h, C.c_void_p(luma.data_ptr()), luma.stride(1), luma.stride(0), w, h, n,
                                               first_frame_no, flags, C.c_void_p(out_lines.data_ptr()), out_lines.shape[0],
                                               C.c_void_p(out_stats.data_ptr()), out_stats.shape[0], sptr)
        self._check(rc)
        return out_lines[:nrec], out_stats[:nst]

    def pcm16x0_binarize_frames(self, luma, first_frame_no: int = 1, new_file: bool = False, doubled: bool = False,
                                out_lines=None, out_stats=None, stream=None, end_file: bool = False):
        """VideoToDigital::doBinarize with setPCMType(TYPE_PCM16X0) over whole frames: luma is a torch.uint8 CUDA tensor
        (n_frames, height, width).  Returns (lines, stats): torch.uint8 CUDA tensors (n_records, 36) of sdv_pcm16x0_bin_rec - three
        per video line, one per service line - and (n_frames, 32) of sdv_frame_stats."""
        import torch
        assert luma.is_cuda and luma.dtype == torch.uint8 and luma.dim() == 3 and luma.stride(2) == 1
        n, h, w = luma.shape
        flags = (FLAG_NEW_FILE if new_file else 0) | (FLAG_DOUBLED if doubled else 0) | (FLAG_END_FILE if end_file else 0)
        nrec = int(self.lib.sdv_pcm16x0_binarize_records(h, n, flags))
        nst = n + (1 if end_file else 0)
        if out_lines is None:
            out_lines = torch.empty((nrec, 36), dtype=torch.uint8, device=luma.device)
        if out_stats is None:
            out_stats = torch.empty((nst, 32), dtype=torch.uint8, device=luma.device)
        _check_out(out_lines, 36, luma.device, "out_lines")
        _check_out(out_stats, 32, luma.device, "out_stats")
        sptr = C.c_void_p(stream.cuda_stream) if stream is not None else C.c_void_p(torch.cuda.current_stream(luma.device).cuda_stream)
        rc = self.lib.sdv_pcm16x0_binarize_frames(self._h, C.c_void_p(luma.data_ptr()), luma.stride(1), luma.stride(0), w, h, n,
                                                  first_frame_no, flags, C.c_void_p(out_lines.data_ptr()), out_lines.shape[0],
                                                  C.c_void_p(out_stats.data_ptr()), out_stats.shape[0], sptr)
        self._check(rc)
        return out_lines[:nrec], out_stats[:nst]

    # ---- batch replacement of doBinarize ----
    def records_per_frame(self, height: int) -> int:
        return int(self.lib.sdv_records_per_frame(height))

    def binarize_frames(self, luma, first_frame_no: int = 1, new_file: bool = False, doubled: bool = False,
                        out_lines=None, out_stats=None, stream=None, end_file: bool = False):
        """luma: torch.uint8 CUDA tensor (n_frames, height, width), rows contiguous.
        Returns (lines, stats) as torch.uint8 CUDA tensors shaped (n_records, 48) and (n_frames, 32)."""
        import torch
        assert luma.is_cuda and luma.dtype == torch.uint8 and luma.dim() == 3 and luma.stride(2) == 1
        n, h, w = luma.shape
        nrec = n * (h + 3) + (1 if new_file else 0) + (h + 4 if end_file else 0)      # end_file: the filler frame that closes a source
        if out_lines is None:
            out_lines = torch.empty((nrec, 48), dtype=torch.uint8, device=luma.device)
        nst = n + (1 if end_file else 0)
        if out_stats is None:
            out_stats = torch.empty((nst, 32), dtype=torch.uint8, device=luma.device)
        _check_out(out_lines, 48, luma.device, "out_lines")
        _check_out(out_stats, 32, luma.device, "out_stats")
        flags = (FLAG_NEW_FILE if new_file else 0) | (FLAG_DOUBLED if doubled else 0) | (FLAG_END_FILE if end_file else 0)
        sptr = C.c_void_p(stream.cuda_stream) if stream is not None else C.c_void_p(torch.cuda.current_stream(luma.device).cuda_stream)
        # the library checks the capacities against what the call will write (SDV_ERR_BAD_ARG when a buffer is too small)
        rc = self.lib.sdv_binarize_frames(self._h, C.c_void_p(luma.data_ptr()), luma.stride(1), luma.stride(0), w, h, n,
                                          first_frame_no, flags, C.c_void_p(out_lines.data_ptr()), out_lines.shape[0],
                                          C.c_void_p(out_stats.data_ptr()), out_stats.shape[0], sptr)
        self._check(rc)
        return out_lines[:nrec], out_stats[:nst]

    # ---- AudioProcessor / SamplesToWAV -----------------------------------------------------------
    def set_audio_masking(self, drop_mode: int):
        """AudioProcessor::setMasking (audioprocessor.cpp:1532-1574): SDV_DROP_* 0..6, and the two modes the reference does not have,
        abi.DROP_INTER_CUBIC_BLOCK (8) and abi.DROP_INTER_CUBIC_WORD (9): cubic interpolation of runs of up to abi.AP_CUBIC_MAX_RUN samples."""
        self._check(self.lib.sdv_set_audio_masking(self._h, int(drop_mode)))

    def reset_audio(self):
        """A freshly constructed AudioProcessor: nothing waits, the sample index is 0; the masking mode stays."""
        self._check(self.lib.sdv_reset_audio(self._h))

    def audio_pending(self) -> int:
        return int(self.lib.sdv_audio_pending(self._h))

    def audio_stalled(self) -> bool:
        """The worker takes no more input: its window is full and the first pairs can never leave (audioprocessor.cpp:108)."""
        return bool(self.lib.sdv_audio_stalled(self._h))

    def audio_next_index(self) -> int:
        return int(self.lib.sdv_audio_next_index(self._h))

    def audio_process(self, pairs, stop=False, out_pairs=None, out_purges=None, stream=None):
        """AudioProcessor::processAudio over one burst of the PCMSamplePair stream: `pairs` is a torch.uint8 CUDA tensor (n, 12) of
        sdv_sample_pair (what the stitch entry points return, tags included).  Returns (out, purges, masked): torch.uint8 CUDA tensors
        (n_out, 12) of sdv_sample_pair and (n_purges, 16) of sdv_audio_purge, and the sum of the guiAddMask reports."""
        import torch
        _check_out(pairs, 12, pairs.device, "pairs")
        n = pairs.shape[0]
        if out_pairs is None:
            out_pairs = torch.empty((n + 1024, 12), dtype=torch.uint8, device=pairs.device)
        if out_purges is None:
            out_purges = torch.empty((256, 16), dtype=torch.uint8, device=pairs.device)
        _check_out(out_pairs, 12, pairs.device, "out_pairs")
        _check_out(out_purges, 16, pairs.device, "out_purges")
        sptr = C.c_void_p(stream.cuda_stream) if stream is not None else C.c_void_p(torch.cuda.current_stream(pairs.device).cuda_stream)
        n_out, n_pur, masked = C.c_size_t(0), C.c_size_t(0), C.c_uint64(0)
        for attempt in range(2):
            rc = self.lib.sdv_audio_process(self._h, C.c_void_p(pairs.data_ptr()) if n else None, n, 1 if stop else 0, C.c_void_p(out_pairs.data_ptr()),
                                            out_pairs.shape[0], C.byref(n_out), C.c_void_p(out_purges.data_ptr()), out_purges.shape[0], C.byref(n_pur),
                                            C.byref(masked), sptr)
            if rc == -1 and attempt == 0 and (n_out.value > out_pairs.shape[0] or n_pur.value > out_purges.shape[0]):
                # a refused call takes nothing: come again with the sizes it reported
                if n_out.value > out_pairs.shape[0]:
                    out_pairs = torch.empty((n_out.value, 12), dtype=torch.uint8, device=pairs.device)
                if n_pur.value > out_purges.shape[0]:
                    out_purges = torch.empty((n_pur.value, 16), dtype=torch.uint8, device=pairs.device)
                continue
            break
        self._check(rc)
        return out_pairs[:n_out.value], out_purges[:n_pur.value], int(masked.value)

    def wav_pack(self, pairs, out=None, stream=None):
        """SamplesToWAV::saveAudio for every pair: (n, 12) sdv_sample_pair -> (n, 2) int16 on the device."""
        import torch
        _check_out(pairs, 12, pairs.device, "pairs")
        n = pairs.shape[0]
        if out is None:
            out = torch.empty((n, 2), dtype=torch.int16, device=pairs.device)
        assert out.is_cuda and out.dtype == torch.int16 and out.is_contiguous() and out.numel() >= 2 * n
        sptr = C.c_void_p(stream.cuda_stream) if stream is not None else C.c_void_p(torch.cuda.current_stream(pairs.device).cuda_stream)
        self._check(self.lib.sdv_wav_pack(self._h, C.c_void_p(pairs.data_ptr()) if n else None, n, C.c_void_p(out.data_ptr()), sptr))
        return out[:n]

    def wav_header(self, n_pairs: int, last_sample_rate: int) -> bytes:
        hdr = C.create_string_buffer(44)
        self.lib.sdv_wav_header(hdr, int(n_pairs), int(last_sample_rate))
        return hdr.raw

    # ---- de-emphasis (50/15 us) of the pair stream: beyond the reference, which leaves it to the user --------------------
    def set_deemphasis(self, mode: int):
        """DEEMPH_OFF (the default) / DEEMPH_AUTO (pairs whose emphasis field is set) / DEEMPH_FORCE (every pair: what an STC-007 tape
        needs, whose chain never sets the field).  Also switches the stage on behind the AudioProcessor of decode_frames(with_audio=True)."""
        self._check(self.lib.sdv_set_deemphasis(self._h, int(mode)))

    def reset_deemphasis(self):
        """The filter forgets the stream it was on: the next selected pair starts a segment (no click)."""
        self._check(self.lib.sdv_reset_deemphasis(self._h))

    def audio_deemphasis(self, pairs, out=None, stream=None):
        """The de-emphasis network over one burst of the stream: (n, 12) sdv_sample_pair -> (n, 12) on the device, asynchronous on the
        stream.  out may be `pairs` itself (in place); the filter state stays in the engine from call to call."""
        import torch
        _check_out(pairs, 12, pairs.device, "pairs")
        n = pairs.shape[0]
        if out is None:
            out = torch.empty((n, 12), dtype=torch.uint8, device=pairs.device)
        _check_out(out, 12, pairs.device, "out")
        assert out.shape[0] >= n
        sptr = C.c_void_p(stream.cuda_stream) if stream is not None else C.c_void_p(torch.cuda.current_stream(pairs.device).cuda_stream)
        self._check(self.lib.sdv_audio_deemphasis(self._h, C.c_void_p(pairs.data_ptr()) if n else None, n, C.c_void_p(out.data_ptr()) if n else None, sptr))
        return out[:n]

    def deemphasis_coeffs(self, rate: int):
        """(b0, b1, a1) of the network at the rate of a pair (44056, anything else reads 44100)."""
        c = (C.c_double * 3)()
        self.lib.sdv_deemphasis_coeffs(int(rate), c)
        return tuple(c)

    # ---- 44 056 Hz -> 44 100 Hz: beyond the reference, which writes the NTSC rate into the WAV header ---------------------
    def set_resample(self, mode: int):
        """RESAMPLE_OFF (the default: audio_resample copies) / RESAMPLE_TO_44100, either with RESAMPLE_DELAY_RIGHT or RESAMPLE_DELAY_LEFT or-ed to it: the
        skew stage behind it delays that channel by half a sample (the PCM-F1 family samples its channels half a period apart; "left first, so delay
        the right channel" is the usual case, not a verified one).  A change of the delay while pairs wait in the skew stage is refused: flush or reset first."""
        self._check(self.lib.sdv_set_resample(self._h, int(mode)))

    def reset_resample(self):
        """No open segment, nothing pending."""
        self._check(self.lib.sdv_reset_resample(self._h))

    def audio_resample_pending(self) -> int:
        return int(self.lib.sdv_audio_resample_pending(self._h))

    def audio_resample(self, pairs, flush=False, out=None, stream=None):
        """One burst of the stream through the 1001 / 1000 resampler: (n, 12) sdv_sample_pair -> (n_out, 12) on the device; segments of
        44 056 Hz pairs leave at 44 100 Hz, everything else as it came.  Without flush the last 64 pairs of an open segment wait in the
        engine for the next call.  With a delay bit in the mode the skew stage runs behind that (behind the copy, with RESAMPLE_OFF): one pair out per
        pair in, the delayed channel's word filtered, up to 63 more pairs waiting.  out: a buffer of at least sdv_audio_resample_room pairs that
        does not overlap `pairs`."""
        import torch
        _check_out(pairs, 12, pairs.device, "pairs")
        n = pairs.shape[0]
        room = int(self.lib.sdv_audio_resample_room(self._h, n))
        if out is None:
            out = torch.empty((room, 12), dtype=torch.uint8, device=pairs.device)
        _check_out(out, 12, pairs.device, "out")
        sptr = C.c_void_p(stream.cuda_stream) if stream is not None else C.c_void_p(torch.cuda.current_stream(pairs.device).cuda_stream)
        n_out = C.c_size_t(0)
        self._check(self.lib.sdv_audio_resample(self._h, C.c_void_p(pairs.data_ptr()) if n else None, n, 1 if flush else 0,
                                                C.c_void_p(out.data_ptr()) if out.shape[0] else None, out.shape[0], C.byref(n_out), sptr))
        return out[:n_out.value]

    def resample_taps(self, phase: int):
        """The 128 taps of a phase (0 .. 1000), or of the skew stage's half-sample row (RESAMPLE_PHASE_HALF), as a tuple of floats."""
        c = (C.c_double * 128)()
        self.lib.sdv_resample_taps(int(phase), c)
        return tuple(c)

    def wav_files(self, out_pairs, purges):
        """The files SamplesToWAV leaves for an output stream of audio_process (one per NEW_FILE purge that is followed by at least one
        pair): {number of the NEW_FILE tag: bytes}.  `purges` as a numpy array of sdv_audio_purge records (or the uint8 tensor)."""
        import numpy as np
        if hasattr(purges, "cpu"):
            purges = purges.cpu().numpy().view(AUDIO_PURGE_DTYPE).reshape(-1)
        files, k, n = {}, 0, out_pairs.shape[0]
        for i, p in enumerate(purges):
            if p["kind"] != 1:
                continue
            a = int(p["first_pair"])
            b = int(purges[i + 1]["first_pair"]) if i + 1 < len(purges) else n
            if b > a:
                pcm = self.wav_pack(out_pairs[a:b])
                rate = int(out_pairs[b - 1].cpu().numpy().view(PAIR_DTYPE)["sample_rate"][0])
                files[k] = self.wav_header(b - a, rate) + pcm.cpu().numpy().tobytes()
            k += 1
        return files

    # ---- the workers back to back (sdv_decode_frames) ---------------------------------------------
    def decode_frames(self, pcm_type: int, luma, first_frame_no: int = 1, new_file: bool = False, doubled: bool = False, end_file: bool = False,
                      with_audio: bool = False, audio_stop: bool = False, stream=None, out_pairs=None, out_frames=None, out_stats=None):
        """Video frames -> PCMSamplePair in one call: the format's VideoToDigital worker, its data stitcher and - with_audio - the AudioProcessor;
        the line records (and the raw pair stream) stay inside the engine.  luma: torch.uint8 CUDA tensor (n_frames, height, width).
        out_pairs / out_frames / out_stats: the caller's buffers ((>= (n + 2) * 1800 + 8192, 12), (>= n + 16, 64 / 52 / 56), (>= n (+ 1), 32) uint8),
        allocated per call when not given.
        Returns (pairs (n, 12), frame descriptors (n, 64 / 52 / 56), frame stats (n, 32)) and, with_audio, also (purges (n, 16), masked)."""
        import torch
        assert luma.is_cuda and luma.dtype == torch.uint8 and luma.dim() == 3 and luma.stride(2) == 1
        n, h, w = luma.shape
        flags = (FLAG_NEW_FILE if new_file else 0) | (FLAG_DOUBLED if doubled else 0) | (FLAG_END_FILE if end_file else 0)
        fr_bytes = {PCM_STC007: 64, 0: 52, 1: 56}[pcm_type]
        nst = n + (1 if end_file else 0)
        if out_pairs is None:
            out_pairs = torch.empty(((n + 2) * 1800 + 8192, 12), dtype=torch.uint8, device=luma.device)
        if out_frames is None:
            out_frames = torch.empty((n + 16, fr_bytes), dtype=torch.uint8, device=luma.device)
        if out_stats is None:
            out_stats = torch.empty((nst, 32), dtype=torch.uint8, device=luma.device)
        for t, cols in ((out_pairs, 12), (out_frames, fr_bytes), (out_stats, 32)):
            assert t.is_cuda and t.dtype == torch.uint8 and t.dim() == 2 and t.shape[1] == cols and t.is_contiguous()
        assert out_stats.shape[0] >= nst
        out_purges = torch.empty((16, 16), dtype=torch.uint8, device=luma.device)
        sptr = C.c_void_p(stream.cuda_stream) if stream is not None else C.c_void_p(torch.cuda.current_stream(luma.device).cuda_stream)
        n_pairs, n_fr, n_pur, masked = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_uint64(0)
        rc = self.lib.sdv_decode_frames(self._h, pcm_type, C.c_void_p(luma.data_ptr()), luma.stride(1), luma.stride(0), w, h, n, first_frame_no, flags,
                                        C.c_void_p(out_pairs.data_ptr()), out_pairs.shape[0], C.byref(n_pairs), C.c_void_p(out_frames.data_ptr()), out_frames.shape[0],
                                        C.byref(n_fr), C.c_void_p(out_stats.data_ptr()), out_stats.shape[0], 1 if with_audio else 0, 1 if audio_stop else 0,
                                        C.c_void_p(out_purges.data_ptr()), out_purges.shape[0], C.byref(n_pur), C.byref(masked), sptr)
        self._check(rc)
        if with_audio:
            return out_pairs[:n_pairs.value], out_frames[:n_fr.value], out_stats[:nst], out_purges[:n_pur.value], int(masked.value)
        return out_pairs[:n_pairs.value], out_frames[:n_fr.value], out_stats[:nst]
