"""include/sdvpcm.h in Python: its POD records, its prototypes and its constants, each stated once.

Everything that calls the C-ABI through ctypes - the Engine, the tests, the tools - takes its structures, numpy dtypes, argtypes and
enum values from here.  The module needs ctypes and numpy only: it loads no library and reads no environment.  tests/test_abi.py pins
every line of it to the header (parameter lists by parsing, layouts and constants through the C compiler)."""
import ctypes as C

import numpy as np

u8, i8, u16, i16, u32, i32, u64, f32 = C.c_uint8, C.c_int8, C.c_uint16, C.c_int16, C.c_uint32, C.c_int32, C.c_uint64, C.c_float


def _f(ctype, names):
    return [(n, ctype) for n in names.split()]


# ---- records: one ctypes.Structure per POD typedef, members named as in the header; the numpy dtypes are derived from them ------------
class LineRec(C.Structure):
    """sdv_line_rec: one binarized STC-007 line"""
    _fields_ = _f(u32, "frame_number") + _f(u16, "line_number") + [("words", u16 * 9)] + _f(u16, "calc_crc") + _f(i16, "data_start data_stop") + \
        _f(u16, "marker_start_bg_coord marker_start_ed_coord marker_stop_ed_coord") + \
        _f(u8, "black_level white_level ref_low ref_level ref_high hysteresis_depth shift_stage service_type mark_st_stage mark_ed_stage flags word_state")


class BinPreset(C.Structure):
    """sdv_bin_preset: bin_preset_t (binarizer.h:163-186)"""
    _fields_ = _f(u8, "max_black_lvl min_white_lvl min_contrast min_ref_lvl max_ref_lvl min_valid_crcs mark_max_dist left_bit_pick right_bit_pick "
                      "en_force_coords en_coord_search en_first_line_dup en_good_no_marker _pad") + _f(i16, "horiz_start horiz_stop")


class BinState(C.Structure):
    """sdv_bin_state: the "good parameters" a Binarizer is preset with (Binarizer::setGoodParameters)"""
    _fields_ = _f(u8, "in_def_black in_def_white in_def_reference do_ref_lvl_sweep") + _f(i16, "in_def_start in_def_stop") + _f(u8, "in_def_from_doubled _pad2")


class FrameStats(C.Structure):
    """sdv_frame_stats: FrameBinDescriptor (frametrimset.h:69-97)"""
    _fields_ = _f(u32, "frame_id") + _f(u16, "line_length lines_odd lines_even lines_pcm_odd lines_pcm_even lines_bad_odd lines_bad_even lines_dup_odd lines_dup_even") + \
        _f(i16, "data_start data_stop") + _f(u8, "data_from_doubled data_not_sure") + [("_pad", u8 * 4)]


class Coord(C.Structure):
    """sdv_coord"""
    _fields_ = _f(i16, "data_start data_stop")


class V2dState(C.Structure):
    """sdv_v2d_state: the frame-to-frame state of VideoToDigital::doBinarize"""
    _fields_ = [("bin", BinState)] + _f(u8, "do_ref_lvl_sweep reset_stats n_last_valid n_long_valid last_valid_doubled_mask_lo last_valid_doubled_mask_hi") + \
        _f(u16, "long_valid_doubled_mask") + [("last_valid", Coord * 9), ("long_valid", Coord * 16), ("_pad", u8 * 2)]


class DeintLine(C.Structure):
    """sdv_deint_line: what STC007Deinterleaver::setWordData reads of one assembled line"""
    _fields_ = _f(u32, "frame_number") + _f(u16, "line_number") + [("words", u16 * 8)] + _f(u8, "word_crc_ok flags")


class DeintSettings(C.Structure):
    """sdv_deint_settings: STC007Deinterleaver settings (stc007deinterleaver.h:151-161)"""
    _fields_ = _f(u8, "res_mode ignore_crc force_ecc_check en_p_code en_q_code en_cwd") + [("_pad", u8 * 2)]


class BlockRec(C.Structure):
    """sdv_block_rec: one STC007DataBlock"""
    _fields_ = [("w_frame", u32 * 8), ("w_line", u16 * 8), ("words", u16 * 8)] + _f(u8, "line_crc cwd_fixed word_valid resolution audio_state cwd_applied") + \
        _f(u16, "sample_rate")


class SamplePair(C.Structure):
    """sdv_sample_pair: PCMSamplePair"""
    _fields_ = [("audio_word", i16 * 2), ("sample_flags", u8 * 2)] + _f(u16, "sample_rate") + _f(u8, "emphasis service_type") + _f(u16, "_pad")


_FRAME_ASM_HEAD = _f(u32, "frame_number") + _f(u16, "odd_std_lines even_std_lines odd_data_lines even_data_lines odd_valid_lines even_valid_lines "
                                                    "odd_top_data odd_bottom_data even_top_data even_bottom_data odd_sample_rate even_sample_rate "
                                                    "blocks_total blocks_drop samples_drop")


class FrameAsm(C.Structure):
    """sdv_frame_asm: FrameAsmSTC007"""
    _fields_ = _FRAME_ASM_HEAD + _f(u16, "inner_padding outer_padding blocks_broken_field blocks_broken_seam blocks_fix_p blocks_fix_q blocks_fix_cwd") + \
        _f(u8, "field_order odd_ref even_ref service_type video_standard tff_cnt bff_cnt odd_resolution even_resolution flags flags2") + \
        _f(i8, "ctrl_index ctrl_hour ctrl_minute ctrl_second ctrl_field")


class StitchSettings(C.Structure):
    """sdv_stitch_settings: STC007DataStitcher settings (slots stc007datastitcher.h:331-350)"""
    _fields_ = _f(u8, "video_standard field_order enable_p enable_q enable_cwd m2_format resolution_preset max_unch_14 max_unch_16 use_ecc mask_seams "
                      "broke_mask top_line_fix _pad") + _f(u16, "sample_rate_preset")


class RunInfo(C.Structure):
    """sdv_run_info: how the last frame entry call was scheduled"""
    _fields_ = _f(u32, "frames rounds frames_launched frames_general") + _f(f32, "kernel_ms") + _f(u32, "sweeps frames_met")


class IngestDesc(C.Structure):
    """sdv_ingest_desc"""
    _fields_ = _f(u8, "pix_fmt colors double_width _pad") + _f(u16, "crop_left crop_right crop_top crop_bottom") + _f(i32, "src_width src_height")


class EncodeDesc(C.Structure):
    """sdv_encode_desc"""
    _fields_ = _f(u8, "video_standard resolution ctrl_block ctrl_flags field_order black white _pad tc_index tc_hour tc_minute tc_second tc_field") + \
        [("out_fmt", u8 * 3)] + _f(i32, "width height data_start data_stop top_line")


class EncodeMarkerlessDesc(C.Structure):
    """sdv_encode_markerless_desc"""
    _fields_ = _f(u8, "format field_order black white header_lines ctrl_flags") + [("out_fmt", u8 * 2)] + _f(i32, "width height data_start data_stop top_line")


class StitchInfo(C.Structure):
    """sdv_stitch_info: how the last stitch call was scheduled"""
    _fields_ = _f(u32, "steps rounds steps_launched pipelined") + _f(f32, "device_ms") + _f(u32, "direct_frames")


_BIN_LEVELS = _f(u8, "black_level white_level ref_low ref_level ref_high hysteresis_depth shift_stage service_type picked_bits_left picked_bits_right flags")


class Pcm1BinRec(C.Structure):
    """sdv_pcm1_bin_rec: one PCM1Line as Binarizer::processLine leaves it"""
    _fields_ = _f(u32, "frame_number") + _f(u16, "line_number") + [("words", u16 * 7)] + _f(u16, "calc_crc") + _f(i16, "data_start data_stop") + _BIN_LEVELS + \
        [("_pad", u8 * 3)]


class Pcm16x0BinRec(C.Structure):
    """sdv_pcm16x0_bin_rec: one PCM16X0SubLine as Binarizer::processLine leaves it"""
    _fields_ = _f(u32, "frame_number") + _f(u16, "line_number") + [("words", u16 * 4)] + _f(u16, "calc_crc") + _f(i16, "data_start data_stop") + \
        _f(u16, "queue_order") + _BIN_LEVELS + _f(u8, "line_part control_bit _pad")


class Pcm1LineRec(C.Structure):
    """sdv_pcm1_line_rec: what PCM1DataStitcher reads of one PCM1Line"""
    _fields_ = _f(u32, "frame_number") + _f(u16, "line_number") + [("words", u16 * 7)] + _f(u16, "calc_crc") + \
        _f(u8, "ref_level picked_bits_left picked_bits_right service_type flags") + [("_pad", u8 * 5)]


class Pcm1StitchSettings(C.Structure):
    """sdv_pcm1_stitch_settings: PCM1DataStitcher settings (slots pcm1datastitcher.h:183-190)"""
    _fields_ = _f(u8, "field_order auto_offset use_ecc") + _f(i8, "odd_offset even_offset") + [("_pad", u8 * 3)]


class FrameAsmPcm1(C.Structure):
    """sdv_frame_asm_pcm1: FrameAsmPCM1"""
    _fields_ = _FRAME_ASM_HEAD + _f(u16, "odd_top_padding odd_bottom_padding even_top_padding even_bottom_padding blocks_fix_bp") + \
        _f(u8, "field_order odd_ref even_ref service_type flags") + [("_pad", u8 * 3)]


class Pcm1BlockRec(C.Structure):
    """sdv_pcm1_block_rec: one PCM1DataBlock as the stitcher hands it to the visualiser"""
    _fields_ = _f(u32, "frame_number") + _f(u16, "start_line stop_line") + _f(u8, "interleave_num flags") + _f(u16, "sample_rate") + \
        [("words", u16 * 184), ("word_flags", u8 * 184), ("_pad", u8 * 12)]


class Pcm1AsmLineRec(C.Structure):
    """sdv_pcm1_asm_line_rec: one PCM1SubLine of the stitcher's queue"""
    _fields_ = _f(u32, "frame_number") + _f(u16, "line_number") + [("words", u16 * 2)] + _f(u8, "picked_bits_left picked_bits_right line_part flags") + \
        [("_pad", u8 * 2)]


class Pcm16x0StitchSettings(C.Structure):
    """sdv_pcm16x0_stitch_settings: PCM16X0DataStitcher settings (slots pcm16x0datastitcher.h:304-314)"""
    _fields_ = _f(u8, "format field_order p_correction use_ecc mask_seams broke_mask") + _f(u16, "sample_rate_preset")


class FrameAsmPcm16x0(C.Structure):
    """sdv_frame_asm_pcm16x0: FrameAsmPCM16x0"""
    _fields_ = _FRAME_ASM_HEAD + _f(u16, "odd_top_padding odd_bottom_padding even_top_padding even_bottom_padding blocks_broken blocks_fix_bp blocks_fix_p blocks_fix_cwd") + \
        _f(u8, "field_order odd_ref even_ref service_type flags _pad")


class Pcm16x0BlockRec(C.Structure):
    """sdv_pcm16x0_block_rec: one PCM16X0DataBlock as the stitcher hands it to the visualiser"""
    _fields_ = [("words", (u16 * 3) * 3)] + _f(u16, "word_crc word_valid") + _f(u8, "picked_left picked_crc") + [("audio_state", u8 * 3)] + _f(u8, "flags") + \
        _f(u16, "sample_rate") + [("_pad", u8 * 2)]


class AudioPurge(C.Structure):
    """sdv_audio_purge: one purgePipeline() of the AudioProcessor"""
    _fields_ = _f(u64, "first_pair") + _f(u32, "tag_index") + _f(u8, "kind") + [("_pad", u8 * 3)]


class AsmLineRec(C.Structure):
    """sdv_asm_line_rec: one assembled STC007Line as the stitcher hands it to the visualiser"""
    _fields_ = _f(u32, "frame_number") + _f(u16, "line_number") + [("words", u16 * 9)] + _f(u16, "calc_crc word_crc_ok word_valid") + _f(u8, "flags _pad")


RECORDS = {"sdv_line_rec": LineRec, "sdv_bin_preset": BinPreset, "sdv_bin_state": BinState, "sdv_frame_stats": FrameStats, "sdv_coord": Coord,
           "sdv_v2d_state": V2dState, "sdv_deint_line": DeintLine, "sdv_deint_settings": DeintSettings, "sdv_block_rec": BlockRec,
           "sdv_sample_pair": SamplePair, "sdv_frame_asm": FrameAsm, "sdv_stitch_settings": StitchSettings, "sdv_run_info": RunInfo,
           "sdv_ingest_desc": IngestDesc, "sdv_encode_desc": EncodeDesc, "sdv_encode_markerless_desc": EncodeMarkerlessDesc, "sdv_stitch_info": StitchInfo,
           "sdv_pcm1_bin_rec": Pcm1BinRec, "sdv_pcm16x0_bin_rec": Pcm16x0BinRec, "sdv_pcm1_line_rec": Pcm1LineRec,
           "sdv_pcm1_stitch_settings": Pcm1StitchSettings, "sdv_frame_asm_pcm1": FrameAsmPcm1, "sdv_pcm1_block_rec": Pcm1BlockRec,
           "sdv_pcm1_asm_line_rec": Pcm1AsmLineRec, "sdv_pcm16x0_stitch_settings": Pcm16x0StitchSettings, "sdv_frame_asm_pcm16x0": FrameAsmPcm16x0,
           "sdv_pcm16x0_block_rec": Pcm16x0BlockRec, "sdv_audio_purge": AudioPurge, "sdv_asm_line_rec": AsmLineRec}

LINE_DTYPE = np.dtype(LineRec)
BIN_STATE_DTYPE = np.dtype(BinState)
# the same ten bytes under the short names the per-line presets are filled in by: a view of BIN_STATE_DTYPE (same offsets and formats), not a second layout.
# It stays only because smoke() in __graft_entry__.py fills presets by these names; once that uses the header's names it can go.
BIN_STATE_SHORT_DTYPE = np.dtype({"names": ["black", "white", "ref", "sweep_flag", "start", "stop", "doubled", "_pad2"],
                                  "formats": [BIN_STATE_DTYPE[n] for n in BIN_STATE_DTYPE.names],
                                  "offsets": [BIN_STATE_DTYPE.fields[n][1] for n in BIN_STATE_DTYPE.names], "itemsize": BIN_STATE_DTYPE.itemsize})
STATS_DTYPE = np.dtype(FrameStats)
V2D_STATE_DTYPE = np.dtype(V2dState)
DEINT_LINE_DTYPE = np.dtype(DeintLine)
BLOCK_DTYPE = np.dtype(BlockRec)
PAIR_DTYPE = np.dtype(SamplePair)
FRAME_ASM_DTYPE = np.dtype(FrameAsm)
PCM1_BIN_DTYPE = np.dtype(Pcm1BinRec)
PCM16X0_BIN_DTYPE = np.dtype(Pcm16x0BinRec)
PCM1_LINE_DTYPE = np.dtype(Pcm1LineRec)
FRAME_ASM_PCM1_DTYPE = np.dtype(FrameAsmPcm1)
PCM1_BLOCK_DTYPE = np.dtype(Pcm1BlockRec)
PCM1_ASM_LINE_DTYPE = np.dtype(Pcm1AsmLineRec)
FRAME_ASM_PCM16X0_DTYPE = np.dtype(FrameAsmPcm16x0)
PCM16X0_BLOCK_DTYPE = np.dtype(Pcm16x0BlockRec)
AUDIO_PURGE_DTYPE = np.dtype(AudioPurge)
ASM_LINE_DTYPE = np.dtype(AsmLineRec)


# ---- constants: the header's enums and #defines without the SDV_ prefix ----------------------------------------------------------------
ABI_VERSION = 14
OK, ERR_NULL_VIDEO, ERR_NULL_PCM, ERR_SHORT_LINE, ERR_NO_COORD, ERR_NULL_LINES, ERR_NULL_BLOCK, ERR_NO_DATA = 0, 1, 2, 3, 4, 16, 17, 18
ERR_BAD_ARG, ERR_HIP, ERR_NO_DEVICE, ERR_UNSUPPORTED = -1, -2, -3, -4
PCM_PCM1, PCM_PCM16X0, PCM_STC007 = 0, 1, 2
MODE_DRAFT, MODE_FAST, MODE_NORMAL, MODE_INSANE = 0, 1, 2, 3
SRV_NO, SRV_NEW_FILE, SRV_END_FILE, SRV_FILLER, SRV_END_FIELD, SRV_END_FRAME, SRV_HEADER_LINE, SRV_CTRL_BLOCK = 0, 1, 2, 3, 4, 5, 6, 7
LF_REF_SWEEPED, LF_COORDS_SWEEPED, LF_BY_EXT_TUNE, LF_BW_SET, LF_COORDS_SET, LF_FORCED_BAD, LF_CRC_VALID, LF_FROM_DOUBLED = 1, 2, 4, 8, 16, 32, 64, 128
WS_WORD_CRC, WS_WORD_VALID = 1, 2
RES_MODE_14BIT, RES_MODE_14BIT_AUTO, RES_MODE_16BIT_AUTO, RES_MODE_16BIT, RES_14BIT, RES_16BIT = 0, 1, 2, 3, 0, 1
AUD_ORIG, AUD_FIX_P, AUD_FIX_Q, AUD_BROKEN, DL_FIXED_BY_CWD, DL_COORDS_BW_OK = 0, 1, 2, 3, 1, 2
SF_BLOCK_OK, SF_WORD_VALID, SF_WORD_FIXED, SF_WORD_MASKED, PAIR_SRV_NO, PAIR_SRV_NEW_FILE, PAIR_SRV_END_FILE = 1, 2, 4, 8, 0, 1, 2
FA_ORDER_PRESET, FA_ORDER_GUESSED, FA_TRIM_OK, FA_INNER_OK, FA_OUTER_OK, FA_INNER_SILENCE, FA_OUTER_SILENCE, FA_VID_STD_PRESET = 1, 2, 4, 8, 16, 32, 64, 128
FA2_ODD_EMPHASIS, FA2_EVEN_EMPHASIS, FA2_VID_STD_GUESSED, FA1_ODD_EMPHASIS, FA1_EVEN_EMPHASIS = 1, 2, 4, 4, 8
FA16_SILENCE, FA16_PADDING_OK, FA16_EI_FORMAT = 16, 32, 64
FLAG_NEW_FILE, FLAG_DOUBLED, FLAG_END_FILE, FRAME_EMPTY = 1, 2, 4, 1
PIX_GRAY8, PIX_UYVY422, PIX_YUYV422, PIX_V210, PIX_GRAY10LE, PIX_RGB24, PIX_BGR24, PIX_RGB0, PIX_BGR0 = 0, 1, 2, 3, 4, 5, 6, 7, 8
COLOR_BW, COLOR_R, COLOR_G, COLOR_B, INGEST_DOUBLE_OFF, INGEST_DOUBLE_ON, INGEST_DOUBLE_AUTO = 0, 1, 2, 3, 0, 1, 2
ENC_NTSC, ENC_PAL, ENC_14BIT, ENC_16BIT, ENC_TFF, ENC_BFF, ENC_CTRL_COPY_PROHIBITED, ENC_CTRL_EMPHASIS = 0, 1, 0, 1, 0, 1, 1, 2
ENC_FMT_PCM1, ENC_FMT_PCM16X0_SI, ENC_FMT_PCM16X0_EI, ENC_ML_EMPHASIS, ENC_ML_RATE_44100, ENC_ML_CODE = 0, 1, 2, 1, 2, 4
P1B_SHORT, P1B_EMPHASIS, P1W_CRC_OK, P1W_PICKED_LEFT, P1W_PICKED_WORD, P1S_BW_SET, P1S_CRC_VALID, P1S_SKIP = 1, 2, 1, 2, 4, 1, 2, 128
P16_FORMAT_AUTO, P16_FORMAT_SI, P16_FORMAT_EI, P16B_EVEN_ORDER, P16B_EI_FORMAT, P16B_EMPHASIS, P16B_CODE = 0, 1, 2, 1, 2, 4, 8
DROP_IGNORE, DROP_MUTE_BLOCK, DROP_MUTE_WORD, DROP_HOLD_BLOCK, DROP_HOLD_WORD, DROP_INTER_LIN_BLOCK, DROP_INTER_LIN_WORD, DROP_MAX = 0, 1, 2, 3, 4, 5, 6, 7
DROP_INTER_CUBIC_BLOCK, DROP_INTER_CUBIC_WORD, AP_CUBIC_MAX_RUN = 8, 9, 6
AP_BUF_SIZE, AP_MIN_VALID_BEFORE, AP_MAX_RAMP_DOWN, AP_MAX_RAMP_UP, AP_PURGE_NEW_FILE, AP_PURGE_END_FILE, AP_PURGE_STOP = 512, 3, 192, 32, 1, 2, 3
DEEMPH_OFF, DEEMPH_AUTO, DEEMPH_FORCE, DEEMPH_TILE, DEEMPH_WARMUP = 0, 1, 2, 1024, 128
RESAMPLE_L, RESAMPLE_M, RESAMPLE_HALF, RESAMPLE_OFF, RESAMPLE_TO_44100 = 1001, 1000, 64, 0, 1
RESAMPLE_DELAY_RIGHT, RESAMPLE_DELAY_LEFT, RESAMPLE_PHASE_HALF = 4, 8, -1
PREEMPH_TILE, PREEMPH_WARMUP, PCM_RESAMPLE_L, PCM_RESAMPLE_M = 1024, 32, 1000, 1001
AL_FORCED_BAD, AL_MARKERS, AL_CRC_VALID = 1, 2, 4
VIS_STC007_LINES, VIS_PCM1_LINES, VIS_PCM16X0_LINES, VIS_STC007_BLOCKS_NTSC, VIS_STC007_BLOCKS_PAL, VIS_STC007_ASM_NTSC, VIS_STC007_ASM_PAL = 0, 1, 2, 3, 4, 5, 6
VIS_PCM1_BLOCKS, VIS_PCM1_ASM, VIS_PCM16X0_BLOCKS, VIS_M2_SAMPLES = 7, 8, 9, 0x100
# every name above with its value, for the test that holds them to the compiler's
CONSTANTS = {n: v for n, v in list(globals().items()) if n.isupper() and isinstance(v, int)}

# names of the package that are not the header's
TYPE_M2 = 3                      # VideoToDigital::TYPE_M2 (videotodigital.h:77): Engine.setPCMType turns it into PCM_STC007 with m2_sample_format
PIX_FORMATS = {n[4:].lower(): v for n, v in CONSTANTS.items() if n.startswith("PIX_")}


# ---- prototypes: {symbol: (restype, argtypes)} in the order of the header --------------------------------------------------------------
# Buffers that callers hand over as integers (tensor.data_ptr(), ndarray.ctypes.data), streams and the engine handle are VP: ctypes takes
# no int for a POINTER(T).  Settings and descriptors passed with byref, and scalar out-parameters, are typed.
I, U, SZ, U16, U32, U64, VP, P = C.c_int, C.c_uint, C.c_size_t, u16, u32, u64, C.c_void_p, C.POINTER
_FRAMES = [VP, VP, SZ, SZ, I, I, I, U32, U, VP, SZ, VP, SZ, VP]
_STITCH = [VP, VP, SZ, VP, SZ, P(SZ), VP, SZ, P(SZ), VP]
_LINES = [VP, VP, SZ, I, SZ, VP, U32, U16, U16, U]
_VIS_FRAMES = [VP, I, VP, SZ, VP, SZ, VP, SZ, VP]

PROTOTYPES = {
    "sdv_engine_create": (VP, [I]),
    "sdv_engine_destroy": (None, [VP]),
    "sdv_last_error": (C.c_char_p, [VP]),
    "sdv_abi_version": (I, []),
    "sdv_default_bin_preset": (None, [P(BinPreset)]),
    "sdv_set_bin_preset": (I, [VP, P(BinPreset)]),
    "sdv_set_mode": (I, [VP, I]),
    "sdv_set_check_line_dup": (I, [VP, I]),
    "sdv_set_pcm_type": (I, [VP, I, I]),
    "sdv_reset_stream": (I, [VP]),
    "sdv_get_chain_state": (I, [VP, VP]),
    "sdv_set_chain_state": (I, [VP, VP]),
    "sdv_pcm16x0_chain_state_size": (SZ, []),
    "sdv_get_pcm16x0_chain_state": (I, [VP, VP, SZ]),
    "sdv_set_pcm16x0_chain_state": (I, [VP, VP, SZ]),
    "sdv_get_run_info": (I, [VP, P(RunInfo)]),
    "sdv_set_profiling": (I, [VP, I]),
    "sdv_set_frame_flags": (I, [VP, VP, SZ]),
    "sdv_needs_double_width": (I, [I]),
    "sdv_double_width": (I, [VP, VP, SZ, I, SZ, VP, SZ, VP]),
    "sdv_ingest_geometry": (I, [P(IngestDesc), P(I), P(I), P(I), P(SZ)]),
    "sdv_ingest_frames": (I, [VP, P(IngestDesc), VP, SZ, SZ, I, VP, SZ, SZ, VP]),
    "sdv_encode_geometry": (I, [P(EncodeDesc), P(SZ), P(I), P(SZ)]),
    "sdv_encode_frames": (I, [VP, P(EncodeDesc), VP, SZ, I, VP, SZ, SZ, VP]),
    "sdv_reset_encoder": (I, [VP]),
    "sdv_encode_markerless_geometry": (I, [P(EncodeMarkerlessDesc), P(SZ), P(I), P(SZ)]),
    "sdv_encode_markerless_frames": (I, [VP, P(EncodeMarkerlessDesc), VP, SZ, I, VP, SZ, SZ, VP]),
    "sdv_records_per_frame": (SZ, [I]),
    "sdv_binarize_records": (SZ, [I, I, U]),
    "sdv_binarize_frames": (I, _FRAMES),
    "sdv_default_deint_settings": (None, [P(DeintSettings)]),
    "sdv_deinterleave_blocks": (I, [VP, VP, SZ, P(DeintSettings), VP, SZ, VP]),
    "sdv_default_stitch_settings": (None, [P(StitchSettings)]),
    "sdv_set_stitch_settings": (I, [VP, P(StitchSettings)]),
    "sdv_reset_stitcher": (I, [VP]),
    "sdv_get_stitch_info": (I, [VP, P(StitchInfo)]),
    "sdv_stitch_state_size": (SZ, []),
    "sdv_get_stitch_state": (I, [VP, VP, SZ]),
    "sdv_set_stitch_state": (I, [VP, VP, SZ]),
    "sdv_saturate_stitch_stats": (I, [VP]),
    "sdv_stitch_frames": (I, _STITCH),
    "sdv_binarize_lines": (I, _LINES + [VP, SZ, VP]),
    "sdv_pcm1_binarize_lines": (I, _LINES + [I, VP, SZ, VP]),
    "sdv_pcm16x0_binarize_lines": (I, _LINES + [I, VP, SZ, VP, VP]),
    "sdv_pcm16x0_binarize_records": (SZ, [I, I, U]),
    "sdv_pcm16x0_binarize_frames": (I, _FRAMES),
    "sdv_pcm1_binarize_frames": (I, _FRAMES),
    "sdv_default_pcm1_stitch_settings": (None, [P(Pcm1StitchSettings)]),
    "sdv_set_pcm1_stitch_settings": (I, [VP, P(Pcm1StitchSettings)]),
    "sdv_pcm1_stitch_frames": (I, _STITCH),
    "sdv_set_pcm1_stitch_block_output": (I, [VP, VP, SZ]),
    "sdv_pcm1_stitch_block_count": (SZ, [VP]),
    "sdv_set_pcm1_stitch_line_output": (I, [VP, VP, SZ]),
    "sdv_pcm1_stitch_line_count": (SZ, [VP]),
    "sdv_pcm1_bin_to_line_recs": (I, [VP, VP, SZ, VP, VP]),
    "sdv_default_pcm16x0_stitch_settings": (None, [P(Pcm16x0StitchSettings)]),
    "sdv_set_pcm16x0_stitch_settings": (I, [VP, P(Pcm16x0StitchSettings)]),
    "sdv_pcm16x0_stitch_state_size": (SZ, []),
    "sdv_get_pcm16x0_stitch_state": (I, [VP, VP, SZ]),
    "sdv_set_pcm16x0_stitch_state": (I, [VP, VP, SZ]),
    "sdv_saturate_pcm16x0_stitch_stats": (I, [VP]),
    "sdv_pcm16x0_stitch_frames": (I, _STITCH),
    "sdv_set_pcm16x0_stitch_block_output": (I, [VP, VP, SZ]),
    "sdv_pcm16x0_stitch_block_count": (SZ, [VP]),
    "sdv_set_pcm16x0_stitch_line_output": (I, [VP, VP, SZ]),
    "sdv_pcm16x0_stitch_line_count": (SZ, [VP]),
    "sdv_set_audio_masking": (I, [VP, I]),
    "sdv_reset_audio": (I, [VP]),
    "sdv_audio_pending": (SZ, [VP]),
    "sdv_audio_stalled": (I, [VP]),
    "sdv_audio_next_index": (U64, [VP]),
    "sdv_audio_process": (I, [VP, VP, SZ, I, VP, SZ, P(SZ), VP, SZ, P(SZ), P(U64), VP]),
    "sdv_wav_pack": (I, [VP, VP, SZ, VP, VP]),
    "sdv_wav_header": (None, [VP, U64, U16]),
    "sdv_deemphasis_coeffs": (None, [U16, P(C.c_double)]),
    "sdv_set_deemphasis": (I, [VP, I]),
    "sdv_reset_deemphasis": (I, [VP]),
    "sdv_audio_deemphasis": (I, [VP, VP, SZ, VP, VP]),
    "sdv_resample_taps": (None, [I, P(C.c_double)]),
    "sdv_set_resample": (I, [VP, I]),
    "sdv_reset_resample": (I, [VP]),
    "sdv_audio_resample_pending": (SZ, [VP]),
    "sdv_audio_resample_room": (SZ, [VP, SZ]),
    "sdv_audio_resample": (I, [VP, VP, SZ, I, VP, SZ, P(SZ), VP]),
    "sdv_preemphasis_coeffs": (None, [U16, P(C.c_double)]),
    "sdv_reset_preemphasis": (I, [VP]),
    "sdv_pcm_preemphasis": (I, [VP, VP, SZ, U16, VP, VP]),
    "sdv_pcm_preemphasis_clipped": (I, [VP, VP, P(U64)]),
    "sdv_pcm_resample_taps": (None, [I, P(C.c_double)]),
    "sdv_reset_pcm_resample": (I, [VP]),
    "sdv_pcm_resample_pending": (SZ, [VP]),
    "sdv_pcm_resample_room": (SZ, [VP, SZ]),
    "sdv_pcm_resample": (I, [VP, VP, SZ, I, VP, SZ, P(SZ), VP]),
    "sdv_decode_frames": (I, [VP, I, VP, SZ, SZ, I, I, I, U32, U, VP, SZ, P(SZ), VP, SZ, P(SZ), VP, SZ, I, I, VP, SZ, P(SZ), P(U64), VP]),
    "sdv_set_stitch_block_output": (I, [VP, VP, SZ]),
    "sdv_stitch_block_count": (SZ, [VP]),
    "sdv_set_stitch_line_output": (I, [VP, VP, SZ]),
    "sdv_stitch_line_count": (SZ, [VP]),
    "sdv_stitch_line_counts": (SZ, [VP, VP, SZ]),
    "sdv_vis_canvas_size": (I, [I, P(U32), P(U32)]),
    "sdv_vis_reset": (I, [VP, I, VP]),
    "sdv_vis_render_lines": (I, [VP, I, VP, SZ, VP, SZ, P(SZ), VP]),
    "sdv_vis_render_blocks": (I, _VIS_FRAMES),
    "sdv_vis_render_asm_lines": (I, _VIS_FRAMES),
}

# exported by developer and emulator builds only
DEV_PROTOTYPES = {
    "sdv_dev_launch_counts": (I, [VP, VP, SZ]),
    "sdv_dev_poisoned": (I, [P(U64), P(U64)]),
    "sdv_dev_peek_fresh": (I, [I, SZ, VP]),
    "sdv_emu_fail_alloc": (I, [I]),
    "sdv_emu_poison_alloc": (I, [I]),
    "sdv_emu_selftest_bursts": (I, [U64, I]),
}


def bind(lib):
    """Sets restype and argtypes of every symbol of the two tables that `lib` exports (a build of an older ABI lacks some) and returns lib."""
    for table in (PROTOTYPES, DEV_PROTOTYPES):
        for name, (restype, argtypes) in table.items():
            if hasattr(lib, name):
                fn = getattr(lib, name)
                fn.restype, fn.argtypes = restype, argtypes
    return lib

