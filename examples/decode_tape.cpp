/*
 * decode_tape.cpp - the drop-in boundary used the way the Qt application would use it: plain C++ host code, the HIP runtime for
 * the buffers, the C-ABI of include/sdvpcm.h for the work.  No Python, no torch.
 *
 *   decode_tape stc007 <luma.raw> <width> <height> <n_frames> <pairs.out> <frames.out>
 *       8-bit luma frames (what VideoInFFMPEG hands to VideoToDigital, vin_ffmpeg.cpp:281-350) -> sdv_binarize_frames
 *       (the VideoToDigital worker's body) -> sdv_stitch_frames (the STC007DataStitcher worker's body) -> PCMSamplePair records
 *   decode_tape pcm1 <lines.raw> <pairs.out> <frames.out>
 *       sdv_pcm1_line_rec records (the PCM1DataStitcher worker's input deque) -> sdv_pcm1_stitch_frames
 *   decode_tape pcm16x0 <luma.raw> <width> <height> <n_frames> <si|ei> <pairs.out> <frames.out>
 *       8-bit luma frames of a PCM-1600/1610/1630 tape -> sdv_pcm16x0_binarize_frames (VideoToDigital with TYPE_PCM16X0) ->
 *       sdv_pcm16x0_stitch_frames (the PCM16X0DataStitcher worker's body); the sub-line records never leave the device
 *
 *   decode_tape wav <luma.raw> <width> <height> <n_frames> <out.wav> [<mask mode 0..6, 8, 9>] [auto|force] [44100] [deskew-r|deskew-l]
 *       the whole chain of the application for an STC-007 file: sdv_binarize_frames -> sdv_stitch_frames -> sdv_audio_process (the
 *       AudioProcessor worker's loop, linear interpolation of dropouts by default; 8 and 9, SDV_DROP_INTER_CUBIC_BLOCK / _WORD, interpolate runs of up to six
 *       samples cubically, which the reference cannot) -> sdv_wav_pack + sdv_wav_header: with the modes 0..6 the file SamplesToWAV
 *       writes, byte for byte; nothing but the luma goes to the device and nothing but the 16-bit PCM comes back.  With `auto` or `force`
 *       the 50/15 us de-emphasis network (sdv_audio_deemphasis) runs on the file's pairs in front of sdv_wav_pack - `force` is the one for
 *       an STC-007 tape recorded with emphasis, whose pairs never carry the flag `auto` goes by; the reference leaves this to an audio editor.
 *       With `44100` the file's pairs - an NTSC tape runs at 44 056 Hz - are resampled to 44 100 Hz (sdv_audio_resample, flush = 1) behind the
 *       de-emphasis, and the header says 44 100 Hz.  With `deskew-r` (or `deskew-l`) the right (left) channel is delayed by half a sample in the
 *       same call (SDV_RESAMPLE_DELAY_RIGHT / _LEFT): the converter of a PCM-F1 samples the two channels half a period apart.  `deskew-r` is the
 *       usual case - left converted first - but not a verified one: listen to a mono fold-down
 *   decode_tape ingest <video.raw> <pixfmt> <src_w> <src_h> <src_row_stride> <n_frames> <l,r,t,b> <bw|r|g|b> <off|on|auto> <luma.out>
 *       captured frames as the video decoder delivers them (pixfmt: gray8 uyvy422 yuyv422 v210 gray10le rgb24 bgr24 rgb0 bgr0; rows
 *       src_row_stride bytes apart, frames src_h rows apart) -> sdv_ingest_frames: crop, channel, 8-bit luma, 2x doubling -> the plane the
 *       other modes read (and, on the device, the plane the frame entries take); prints `out_w out_h doubled`
 *   decode_tape encode <in.wav> <out.luma> [pal] [16] [noctrl] [emphasis] [nocopy] [from44100] [preemph] [<pixfmt>]
 *       the way back: a 16-bit stereo PCM WAV file -> sdv_encode_frames -> 8-bit luma frames of an STC-007 tape (`16`: PCM-F1, 16 bit) as the
 *       other modes read them: 720 pixels wide, data window 12 .. 708, every line of both fields (NTSC 492 rows, PAL 590; with `noctrl`, without
 *       the control line, 490 / 588), top field first, black 30, white 200.  One frame more than the samples fill is made from no pairs: it plays
 *       the 112 lines of interleave delay out.  `emphasis` and `nocopy` set the bits of the control block (`emphasis` alone leaves the samples as they are).
 *       Prints `n_frames width height row_bytes`; `decode_tape wav <out.luma> 720 <height> <n_frames> <back.wav>` gives the samples back.
 *       <pixfmt>, one of uyvy422 yuyv422 v210 gray10le rgb24 bgr24 rgb0 bgr0: the frames leave the encoder in that packed format (out_fmt of the
 *       descriptor) with neutral chroma, as a playout card or a video encoder takes them: rows of row_bytes bytes with no padding, row_bytes being
 *       the fourth number printed - the stride for the next tool.  `decode_tape ingest <out> <pixfmt> 720 <height> <row_bytes> <n_frames> 0,0,0,0
 *       bw off <luma>` is the way back to the plane `wav` and `frames` read
 *       `from44100`: the file is an ordinary 44 100 Hz WAV and the tape runs at 44 056 Hz - its pairs are resampled before anything else
 *       (sdv_pcm_resample, one call, flush = 1); a usage error with `pal`, whose tape runs at 44 100 Hz.  `preemph`: the pairs are pre-emphasised at
 *       the tape's rate (sdv_pcm_preemphasis; 44 056 Hz, with `pal` 44 100 Hz) and the emphasis bit is set; `clipped N` on stderr says how many samples
 *       that clipped.  `16 from44100 preemph`, then `decode_tape wav ... force 44100`, gives a 44 100 Hz file back
 *   decode_tape encode <in.wav> <out.luma> pcm1|pcm16si|pcm16ei [bff] [emphasis] [44100] [from44100] [preemph] [<pixfmt>]
 *       the same for the marker-less formats: -> sdv_encode_markerless_frames -> frames of a PCM-1 tape (492 rows: one Header line and the 245
 *       data lines of either field) or of a PCM-1630 tape in the SI or EI interleave (490 rows), 720 pixels wide, data window 4 .. 716, black 30,
 *       white 200, top field first or, with `bff`, bottom field first.  `emphasis` and `44100` set Control Bits of a PCM-16x0 tape (without
 *       `44100` it says 44 056 Hz).  As many frames as the samples fill, the rest of the last one silence.  Prints `n_frames width height
 *       row_bytes`; <pixfmt> as above.
 *       `from44100` and `preemph` as above: the tape's rate is 44 056 Hz, or 44 100 Hz for PCM-16x0 with `44100` (with which `from44100` is a usage
 *       error); `preemph` sets the emphasis Control Bit of a PCM-16x0 tape - a PCM-1 tape has none, only its samples change
 *   decode_tape frames <luma.raw> <width> <height> <n_frames> pcm1|pcm16si|pcm16ei tff|bff <pairs.out>
 *       8-bit luma frames of a marker-less format -> sdv_decode_frames (NEW_FILE | END_FILE, no audio stage) -> PCMSamplePair records: what reads
 *       the tapes of `encode` back
 *
 * Build (host code only, any C++ compiler): g++ -std=c++17 -O2 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude examples/decode_tape.cpp
 *        -Lsdvpcmdecoder_amd -lsdvpcm_hip -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,'$ORIGIN/../sdvpcmdecoder_amd' (build.py: build_example).
 */
#include <hip/hip_runtime_api.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "sdvpcm.h"

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)
#define SDV_OKAY(x) do { int r_ = (x); if (r_ != SDV_OK) { fprintf(stderr, "%s = %d: %s\n", #x, r_, sdv_last_error(eng)); return 3; } } while (0)

/* an option of `encode` that names an output pixel format: its SDV_PIX_* value, or -1 */
static int encode_pix_fmt(const std::string &opt)
{
    static const char *const fmts[] = { "gray8", "uyvy422", "yuyv422", "v210", "gray10le", "rgb24", "bgr24", "rgb0", "bgr0" };
    for (int i = 1; i < 9; i++) if (opt == fmts[i]) return i;
    return -1;
}

static bool read_file(const char *path, std::vector<uint8_t> &out)
{
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET);
    out.resize((size_t)n);
    bool ok = fread(out.data(), 1, (size_t)n, f) == (size_t)n;
    fclose(f);
    return ok;
}
static bool write_file(const char *path, const void *p, size_t n)
{
    FILE *f = fopen(path, "wb");
    if (!f) return false;
    bool ok = fwrite(p, 1, n, f) == n;
    fclose(f);
    return ok;
}
/* the data chunk of a RIFF/WAVE file with 16-bit stereo PCM: where its pairs begin in `in`, and how many there are */
static bool read_wav(const char *path, std::vector<uint8_t> &in, size_t *data_at, size_t *n_pairs)
{
    if (!read_file(path, in) || in.size() < 12 || memcmp(in.data(), "RIFF", 4) || memcmp(in.data() + 8, "WAVE", 4)) { fprintf(stderr, "cannot read %s as a WAV file\n", path); return false; }
    size_t at = 12, data_len = 0; unsigned channels = 0, bits = 0;
    *data_at = 0;
    while (at + 8 <= in.size()) {
        const size_t len = (size_t)in[at + 4] | (size_t)in[at + 5] << 8 | (size_t)in[at + 6] << 16 | (size_t)in[at + 7] << 24;
        if (!memcmp(in.data() + at, "fmt ", 4) && at + 8 + 16 <= in.size()) { channels = in[at + 10] | in[at + 11] << 8; bits = in[at + 22] | in[at + 23] << 8; }
        if (!memcmp(in.data() + at, "data", 4)) { *data_at = at + 8; data_len = len < in.size() - *data_at ? len : in.size() - *data_at; break; }
        at += 8 + len + (len & 1);
    }
    if (!*data_at || channels != 2 || bits != 16) { fprintf(stderr, "%s: 16-bit stereo PCM is what a tape holds\n", path); return false; }
    *n_pairs = data_len / 4;
    return true;
}
/* `from44100` and `preemph` of the encode modes, on the file's pairs on the device: resampled to 44 056 Hz (one call, flush = 1), then pre-emphasised
 * at the tape's rate.  *d_pcm and *n become what the encoder reads. */
static int condition_pcm(sdv_engine *eng, int16_t **d_pcm, size_t *n, bool from44100, bool preemph, uint16_t tape_rate)
{
    if (from44100 && *n) {
        const size_t cap = sdv_pcm_resample_room(eng, *n);
        int16_t *d_out = NULL; size_t n_out = 0;
        HIP_OK(hipMalloc((void **)&d_out, cap * 4 + 4));
        SDV_OKAY(sdv_pcm_resample(eng, *d_pcm, *n, 1, d_out, cap, &n_out, NULL));
        HIP_OK(hipDeviceSynchronize());
        (void)hipFree(*d_pcm); *d_pcm = d_out; *n = n_out;
    }
    if (preemph && *n) {
        int16_t *d_out = NULL; uint64_t clipped = 0;
        HIP_OK(hipMalloc((void **)&d_out, *n * 4 + 4));
        SDV_OKAY(sdv_pcm_preemphasis(eng, *d_pcm, *n, tape_rate, d_out, NULL));
        SDV_OKAY(sdv_pcm_preemphasis_clipped(eng, NULL, &clipped));
        if (clipped) fprintf(stderr, "clipped %llu\n", (unsigned long long)clipped);
        (void)hipFree(*d_pcm); *d_pcm = d_out;
    }
    return 0;
}
template <class T> static int download(const T *dev, size_t n, const char *path)
{
    std::vector<T> host(n);
    if (n) HIP_OK(hipMemcpy(host.data(), dev, n * sizeof(T), hipMemcpyDeviceToHost));
    return write_file(path, host.data(), n * sizeof(T)) ? 0 : 4;
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: see the header of examples/decode_tape.cpp\n"); return 1; }
    const std::string mode = argv[1];
    sdv_engine *eng = sdv_engine_create(0);
    if (!eng) { fprintf(stderr, "sdv_engine_create: %s\n", sdv_last_error(NULL)); return 2; }
    std::vector<uint8_t> in;
    sdv_sample_pair *d_pairs = NULL;
    size_t n_pairs = 0, n_frames = 0;
    int rc = 0;
    /* wav: the optional last words, `auto|force`, behind it `44100` and behind that `deskew-r|deskew-l` */
    const bool wav = mode == "wav";
    const std::string skew_arg = wav ? argv[argc - 1] : "";
    const int deskew = skew_arg == "deskew-r" ? SDV_RESAMPLE_DELAY_RIGHT : skew_arg == "deskew-l" ? SDV_RESAMPLE_DELAY_LEFT : 0, skew_words = deskew ? 1 : 0;
    const int resample = wav && argc - skew_words > 2 && std::string(argv[argc - 1 - skew_words]) == "44100" ? 1 : 0;
    const std::string last_arg = wav && argc - skew_words - resample > 2 ? argv[argc - 1 - skew_words - resample] : "";
    const int deemph = last_arg == "auto" ? SDV_DEEMPH_AUTO : last_arg == "force" ? SDV_DEEMPH_FORCE : SDV_DEEMPH_OFF, wav_tail = (deemph != SDV_DEEMPH_OFF ? 1 : 0) + resample + skew_words;
    if (mode == "stc007" && argc == 8) {
        const int width = atoi(argv[3]), height = atoi(argv[4]), n = atoi(argv[5]);
        if (!read_file(argv[2], in) || in.size() != (size_t)width * height * n) { fprintf(stderr, "cannot read %s\n", argv[2]); return 1; }
        uint8_t *d_luma = NULL; sdv_line_rec *d_lines = NULL; sdv_frame_stats *d_stats = NULL; sdv_frame_asm *d_frames = NULL;
        /* one file from its first to its last frame: NEW_FILE tag ahead, filler frame + END_FILE tag behind */
        const size_t n_lines = sdv_binarize_records(height, n, SDV_FLAG_NEW_FILE | SDV_FLAG_END_FILE);
        const size_t pairs_cap = n_lines * 4 + 8192, frames_cap = (size_t)n + 16;
        HIP_OK(hipMalloc((void **)&d_luma, in.size()));
        HIP_OK(hipMalloc((void **)&d_lines, n_lines * sizeof(sdv_line_rec)));
        HIP_OK(hipMalloc((void **)&d_stats, ((size_t)n + 1) * sizeof(sdv_frame_stats)));
        HIP_OK(hipMalloc((void **)&d_pairs, pairs_cap * sizeof(sdv_sample_pair)));
        HIP_OK(hipMalloc((void **)&d_frames, frames_cap * sizeof(sdv_frame_asm)));
        HIP_OK(hipMemcpy(d_luma, in.data(), in.size(), hipMemcpyHostToDevice));
        SDV_OKAY(sdv_set_mode(eng, SDV_MODE_NORMAL));
        SDV_OKAY(sdv_binarize_frames(eng, d_luma, (size_t)width, (size_t)width * height, width, height, n, 1,
                                     SDV_FLAG_NEW_FILE | SDV_FLAG_END_FILE, d_lines, n_lines, d_stats, (size_t)n + 1, NULL));
        sdv_stitch_settings st; sdv_default_stitch_settings(&st);
        SDV_OKAY(sdv_set_stitch_settings(eng, &st));
        SDV_OKAY(sdv_stitch_frames(eng, d_lines, n_lines, d_pairs, pairs_cap, &n_pairs, d_frames, frames_cap, &n_frames, NULL));
        HIP_OK(hipDeviceSynchronize());
        rc = download(d_pairs, n_pairs, argv[6]); if (!rc) rc = download(d_frames, n_frames, argv[7]);
        sdv_run_info info; sdv_get_run_info(eng, &info);
        printf("stc007: %d frames -> %zu line records -> %zu sample pairs, %zu frame descriptors (binarize rounds %u)\n", n, n_lines, n_pairs, n_frames, info.rounds);
        (void)hipFree(d_luma); (void)hipFree(d_lines); (void)hipFree(d_stats); (void)hipFree(d_frames);
    } else if (wav && (argc - wav_tail == 7 || argc - wav_tail == 8)) {
        const int width = atoi(argv[3]), height = atoi(argv[4]), n = atoi(argv[5]);
        const int mask_mode = argc - wav_tail == 8 ? atoi(argv[7]) : SDV_DROP_INTER_LIN_WORD;
        if (!read_file(argv[2], in) || in.size() != (size_t)width * height * n) { fprintf(stderr, "cannot read %s\n", argv[2]); return 1; }
        uint8_t *d_luma = NULL; sdv_line_rec *d_lines = NULL; sdv_frame_stats *d_stats = NULL; sdv_frame_asm *d_frames = NULL;
        sdv_sample_pair *d_audio = NULL, *d_resampled = NULL; sdv_audio_purge *d_purges = NULL; int16_t *d_pcm = NULL;
        const size_t n_lines = sdv_binarize_records(height, n, SDV_FLAG_NEW_FILE | SDV_FLAG_END_FILE);
        const size_t pairs_cap = n_lines * 4 + 8192, frames_cap = (size_t)n + 16, purges_cap = 8;
        HIP_OK(hipMalloc((void **)&d_luma, in.size()));
        HIP_OK(hipMalloc((void **)&d_lines, n_lines * sizeof(sdv_line_rec)));
        HIP_OK(hipMalloc((void **)&d_stats, ((size_t)n + 1) * sizeof(sdv_frame_stats)));
        HIP_OK(hipMalloc((void **)&d_pairs, pairs_cap * sizeof(sdv_sample_pair)));
        HIP_OK(hipMalloc((void **)&d_frames, frames_cap * sizeof(sdv_frame_asm)));
        HIP_OK(hipMalloc((void **)&d_audio, (pairs_cap + 1024) * sizeof(sdv_sample_pair)));
        HIP_OK(hipMalloc((void **)&d_purges, purges_cap * sizeof(sdv_audio_purge)));
        /* with `44100` and / or `deskew-*`: room for every pair of the audio stage through sdv_audio_resample (the bound grows with the pairs of the call) */
        const int rs_mode = (resample ? SDV_RESAMPLE_TO_44100 : SDV_RESAMPLE_OFF) | deskew;
        if (rs_mode) SDV_OKAY(sdv_set_resample(eng, rs_mode));
        const size_t res_cap = sdv_audio_resample_room(eng, pairs_cap + 1024);
        if (rs_mode) HIP_OK(hipMalloc((void **)&d_resampled, res_cap * sizeof(sdv_sample_pair)));
        HIP_OK(hipMalloc((void **)&d_pcm, res_cap * 2 * sizeof(int16_t)));
        HIP_OK(hipMemcpy(d_luma, in.data(), in.size(), hipMemcpyHostToDevice));
        SDV_OKAY(sdv_set_mode(eng, SDV_MODE_NORMAL));
        SDV_OKAY(sdv_binarize_frames(eng, d_luma, (size_t)width, (size_t)width * height, width, height, n, 1,
                                     SDV_FLAG_NEW_FILE | SDV_FLAG_END_FILE, d_lines, n_lines, d_stats, (size_t)n + 1, NULL));
        sdv_stitch_settings st; sdv_default_stitch_settings(&st);
        SDV_OKAY(sdv_set_stitch_settings(eng, &st));
        SDV_OKAY(sdv_stitch_frames(eng, d_lines, n_lines, d_pairs, pairs_cap, &n_pairs, d_frames, frames_cap, &n_frames, NULL));
        /* the pair stream (NEW_FILE ... END_FILE) stays on the device and goes straight into the audio stage; stop = the application closing */
        size_t n_audio = 0, n_purges = 0; uint64_t n_masked = 0;
        SDV_OKAY(sdv_set_audio_masking(eng, mask_mode));
        SDV_OKAY(sdv_audio_process(eng, d_pairs, n_pairs, 1, d_audio, pairs_cap + 1024, &n_audio, d_purges, purges_cap, &n_purges, &n_masked, NULL));
        std::vector<sdv_audio_purge> purges(n_purges);
        if (n_purges) HIP_OK(hipMemcpy(purges.data(), d_purges, n_purges * sizeof(sdv_audio_purge), hipMemcpyDeviceToHost));
        /* the file of the first source: the pairs between its NEW_FILE purge and the next purge */
        size_t a = 0, b = 0; bool found = false;
        for (size_t k = 0; k < n_purges && !found; k++) if (purges[k].kind == SDV_AP_PURGE_NEW_FILE) { a = (size_t)purges[k].first_pair; b = k + 1 < n_purges ? (size_t)purges[k + 1].first_pair : n_audio; found = true; }
        if (!found || b <= a) { fprintf(stderr, "no audio came out\n"); rc = 5; }
        else {
            if (deemph != SDV_DEEMPH_OFF) {         /* in place, on what goes into the file */
                SDV_OKAY(sdv_set_deemphasis(eng, deemph));
                SDV_OKAY(sdv_audio_deemphasis(eng, d_audio + a, b - a, d_audio + a, NULL));
            }
            const sdv_sample_pair *d_file = d_audio + a; size_t n_file = b - a;
            if (rs_mode) {                          /* the file's range, closed behind its last pair */
                size_t n_res = 0;
                SDV_OKAY(sdv_audio_resample(eng, d_file, n_file, 1, d_resampled, res_cap, &n_res, NULL));
                d_file = d_resampled; n_file = n_res;
            }
            SDV_OKAY(sdv_wav_pack(eng, d_file, n_file, d_pcm, NULL));
            HIP_OK(hipDeviceSynchronize());
            sdv_sample_pair last;
            HIP_OK(hipMemcpy(&last, d_file + (n_file - 1), sizeof(last), hipMemcpyDeviceToHost));
            std::vector<uint8_t> file(44 + 4 * n_file);
            sdv_wav_header(file.data(), n_file, last.sample_rate);
            HIP_OK(hipMemcpy(file.data() + 44, d_pcm, 4 * n_file, hipMemcpyDeviceToHost));
            rc = write_file(argv[6], file.data(), file.size()) ? 0 : 4;
            printf("wav: %d frames -> %zu sample pairs -> %zu after the audio stage (%llu samples masked, %zu purges) -> %zu bytes at %u Hz\n", n, n_pairs, n_audio,
                   (unsigned long long)n_masked, n_purges, file.size(), last.sample_rate == 44056 ? 44056u : 44100u);
        }
        (void)hipFree(d_luma); (void)hipFree(d_lines); (void)hipFree(d_stats); (void)hipFree(d_frames); (void)hipFree(d_audio); (void)hipFree(d_purges); (void)hipFree(d_pcm); (void)hipFree(d_resampled);
    } else if (mode == "pcm1" && argc == 5) {
        if (!read_file(argv[2], in) || in.size() % sizeof(sdv_pcm1_line_rec)) { fprintf(stderr, "cannot read %s\n", argv[2]); return 1; }
        const size_t n_lines = in.size() / sizeof(sdv_pcm1_line_rec);
        sdv_pcm1_line_rec *d_lines = NULL; sdv_frame_asm_pcm1 *d_frames = NULL;
        const size_t pairs_cap = n_lines * 3 + 4096, frames_cap = n_lines / 32 + 64;
        HIP_OK(hipMalloc((void **)&d_lines, in.size() ? in.size() : 32));
        HIP_OK(hipMalloc((void **)&d_pairs, pairs_cap * sizeof(sdv_sample_pair)));
        HIP_OK(hipMalloc((void **)&d_frames, frames_cap * sizeof(sdv_frame_asm_pcm1)));
        HIP_OK(hipMemcpy(d_lines, in.data(), in.size(), hipMemcpyHostToDevice));
        sdv_pcm1_stitch_settings st; sdv_default_pcm1_stitch_settings(&st);
        SDV_OKAY(sdv_set_pcm1_stitch_settings(eng, &st));
        SDV_OKAY(sdv_pcm1_stitch_frames(eng, d_lines, n_lines, d_pairs, pairs_cap, &n_pairs, d_frames, frames_cap, &n_frames, NULL));
        HIP_OK(hipDeviceSynchronize());
        rc = download(d_pairs, n_pairs, argv[3]); if (!rc) rc = download(d_frames, n_frames, argv[4]);
        printf("pcm1: %zu line records -> %zu sample pairs, %zu frame descriptors\n", n_lines, n_pairs, n_frames);
        (void)hipFree(d_lines); (void)hipFree(d_frames);
    } else if (mode == "pcm16x0" && argc == 9) {
        const int width = atoi(argv[3]), height = atoi(argv[4]), n = atoi(argv[5]);
        const bool ei = std::string(argv[6]) == "ei";
        if (!read_file(argv[2], in) || in.size() != (size_t)width * height * n) { fprintf(stderr, "cannot read %s\n", argv[2]); return 1; }
        uint8_t *d_luma = NULL; sdv_pcm16x0_bin_rec *d_lines = NULL; sdv_frame_stats *d_stats = NULL; sdv_frame_asm_pcm16x0 *d_frames = NULL;
        const unsigned flags = SDV_FLAG_NEW_FILE | SDV_FLAG_END_FILE;
        const size_t n_lines = sdv_pcm16x0_binarize_records(height, n, flags);
        const size_t pairs_cap = (size_t)(n + 1) * 1470 + 16, frames_cap = (size_t)n + 16;
        HIP_OK(hipMalloc((void **)&d_luma, in.size()));
        HIP_OK(hipMalloc((void **)&d_lines, n_lines * sizeof(sdv_pcm16x0_bin_rec)));
        HIP_OK(hipMalloc((void **)&d_stats, ((size_t)n + 1) * sizeof(sdv_frame_stats)));
        HIP_OK(hipMalloc((void **)&d_pairs, pairs_cap * sizeof(sdv_sample_pair)));
        HIP_OK(hipMalloc((void **)&d_frames, frames_cap * sizeof(sdv_frame_asm_pcm16x0)));
        HIP_OK(hipMemcpy(d_luma, in.data(), in.size(), hipMemcpyHostToDevice));
        SDV_OKAY(sdv_set_pcm_type(eng, SDV_PCM_PCM16X0, 0));
        SDV_OKAY(sdv_set_mode(eng, SDV_MODE_NORMAL));
        SDV_OKAY(sdv_pcm16x0_binarize_frames(eng, d_luma, (size_t)width, (size_t)width * height, width, height, n, 1, flags, d_lines, n_lines,
                                             d_stats, (size_t)n + 1, NULL));
        sdv_pcm16x0_stitch_settings st; sdv_default_pcm16x0_stitch_settings(&st);
        st.format = ei ? SDV_P16_FORMAT_EI : SDV_P16_FORMAT_SI;
        SDV_OKAY(sdv_set_pcm16x0_stitch_settings(eng, &st));
        SDV_OKAY(sdv_pcm16x0_stitch_frames(eng, d_lines, n_lines, d_pairs, pairs_cap, &n_pairs, d_frames, frames_cap, &n_frames, NULL));
        HIP_OK(hipDeviceSynchronize());
        rc = download(d_pairs, n_pairs, argv[7]); if (!rc) rc = download(d_frames, n_frames, argv[8]);
        sdv_run_info info; sdv_get_run_info(eng, &info);
        printf("pcm16x0 (%s): %d frames -> %zu sub-line records -> %zu sample pairs, %zu frame descriptors (binarize rounds %u)\n", ei ? "EI" : "SI", n, n_lines, n_pairs, n_frames, info.rounds);
        (void)hipFree(d_luma); (void)hipFree(d_lines); (void)hipFree(d_stats); (void)hipFree(d_frames);
    } else if (mode == "ingest" && argc == 12) {
        static const char *const fmts[] = { "gray8", "uyvy422", "yuyv422", "v210", "gray10le", "rgb24", "bgr24", "rgb0", "bgr0" };
        static const char *const cols[] = { "bw", "r", "g", "b" }, *const dbls[] = { "off", "on", "auto" };
        sdv_ingest_desc d; memset(&d, 0, sizeof(d));
        int fmt = -1, col = -1, dbl = -1, crop[4] = { -1, -1, -1, -1 };
        for (int i = 0; i < 9; i++) if (fmts[i] == std::string(argv[3])) fmt = i;
        for (int i = 0; i < 4; i++) if (cols[i] == std::string(argv[9])) col = i;
        for (int i = 0; i < 3; i++) if (dbls[i] == std::string(argv[10])) dbl = i;
        const int n_crop = sscanf(argv[8], "%d,%d,%d,%d", &crop[0], &crop[1], &crop[2], &crop[3]);
        const long stride = atol(argv[6]); const int n = atoi(argv[7]);
        if (fmt < 0 || col < 0 || dbl < 0 || n_crop != 4 || crop[0] < 0 || crop[1] < 0 || crop[2] < 0 || crop[3] < 0 || crop[0] > 65535 || crop[1] > 65535 ||
            crop[2] > 65535 || crop[3] > 65535 || stride <= 0 || n <= 0) { fprintf(stderr, "usage: see the header of examples/decode_tape.cpp\n"); return 1; }
        d.pix_fmt = (uint8_t)fmt; d.colors = (uint8_t)col; d.double_width = (uint8_t)dbl;
        d.crop_left = (uint16_t)crop[0]; d.crop_right = (uint16_t)crop[1]; d.crop_top = (uint16_t)crop[2]; d.crop_bottom = (uint16_t)crop[3];
        d.src_width = atoi(argv[4]); d.src_height = atoi(argv[5]);
        int out_w = 0, out_h = 0, doubled = 0; size_t row_bytes = 0;
        const int grc = sdv_ingest_geometry(&d, &out_w, &out_h, &doubled, &row_bytes);
        if (grc != SDV_OK) { fprintf(stderr, "sdv_ingest_geometry = %d: %s\n", grc, sdv_last_error(NULL)); return 3; }
        const size_t frame_bytes = (size_t)stride * (size_t)d.src_height;
        if (!read_file(argv[2], in) || in.size() != frame_bytes * (size_t)n) { fprintf(stderr, "cannot read %s\n", argv[2]); return 1; }
        uint8_t *d_video = NULL, *d_luma = NULL;
        const size_t luma_bytes = (size_t)out_w * out_h * n;
        HIP_OK(hipMalloc((void **)&d_video, in.size()));
        HIP_OK(hipMalloc((void **)&d_luma, luma_bytes));
        HIP_OK(hipMemcpy(d_video, in.data(), in.size(), hipMemcpyHostToDevice));
        SDV_OKAY(sdv_ingest_frames(eng, &d, d_video, (size_t)stride, frame_bytes, n, d_luma, (size_t)out_w, (size_t)out_w * out_h, NULL));
        HIP_OK(hipDeviceSynchronize());
        rc = download(d_luma, luma_bytes, argv[11]);
        printf("%d %d %d\n", out_w, out_h, doubled);
        (void)hipFree(d_video); (void)hipFree(d_luma);
    } else if (mode == "frames" && argc == 9) {
        const int width = atoi(argv[3]), height = atoi(argv[4]), n = atoi(argv[5]);
        const std::string fmt = argv[6], order = argv[7];
        const int pcm_type = fmt == "pcm1" ? SDV_PCM_PCM1 : fmt == "pcm16si" || fmt == "pcm16ei" ? SDV_PCM_PCM16X0 : -1;
        if (pcm_type < 0 || (order != "tff" && order != "bff") || n <= 0) { fprintf(stderr, "usage: see the header of examples/decode_tape.cpp\n"); return 1; }
        if (!read_file(argv[2], in) || in.size() != (size_t)width * height * n) { fprintf(stderr, "cannot read %s\n", argv[2]); return 1; }
        const uint8_t field_order = order == "bff" ? 2 : 1;
        SDV_OKAY(sdv_set_pcm_type(eng, pcm_type, 0));
        SDV_OKAY(sdv_set_mode(eng, SDV_MODE_NORMAL));
        size_t frame_bytes = 0;
        if (pcm_type == SDV_PCM_PCM1) {
            sdv_pcm1_stitch_settings st; sdv_default_pcm1_stitch_settings(&st);
            st.field_order = field_order;
            SDV_OKAY(sdv_set_pcm1_stitch_settings(eng, &st));
            frame_bytes = sizeof(sdv_frame_asm_pcm1);
        } else {
            sdv_pcm16x0_stitch_settings st; sdv_default_pcm16x0_stitch_settings(&st);
            st.format = fmt == "pcm16ei" ? SDV_P16_FORMAT_EI : SDV_P16_FORMAT_SI; st.field_order = field_order;
            SDV_OKAY(sdv_set_pcm16x0_stitch_settings(eng, &st));
            frame_bytes = sizeof(sdv_frame_asm_pcm16x0);
        }
        uint8_t *d_luma = NULL; void *d_frames = NULL;
        const size_t pairs_cap = ((size_t)n + 2) * 2100 + 8192, frames_cap = (size_t)n + 16;
        HIP_OK(hipMalloc((void **)&d_luma, in.size()));
        HIP_OK(hipMalloc((void **)&d_pairs, pairs_cap * sizeof(sdv_sample_pair)));
        HIP_OK(hipMalloc(&d_frames, frames_cap * frame_bytes));
        HIP_OK(hipMemcpy(d_luma, in.data(), in.size(), hipMemcpyHostToDevice));
        SDV_OKAY(sdv_decode_frames(eng, pcm_type, d_luma, (size_t)width, (size_t)width * height, width, height, n, 1, SDV_FLAG_NEW_FILE | SDV_FLAG_END_FILE,
                                   d_pairs, pairs_cap, &n_pairs, d_frames, frames_cap, &n_frames, NULL, 0, 0, 0, NULL, 0, NULL, NULL, NULL));
        HIP_OK(hipDeviceSynchronize());
        rc = download(d_pairs, n_pairs, argv[8]);
        printf("frames (%s, %s): %d frames -> %zu sample pairs, %zu frame descriptors\n", fmt.c_str(), order.c_str(), n, n_pairs, n_frames);
        (void)hipFree(d_luma); (void)hipFree(d_frames);
    } else if (mode == "encode" && argc >= 5 && (!strcmp(argv[4], "pcm1") || !strcmp(argv[4], "pcm16si") || !strcmp(argv[4], "pcm16ei"))) {
        sdv_encode_markerless_desc d; memset(&d, 0, sizeof(d));
        const bool pcm1 = !strcmp(argv[4], "pcm1");
        d.format = pcm1 ? SDV_ENC_FMT_PCM1 : !strcmp(argv[4], "pcm16si") ? SDV_ENC_FMT_PCM16X0_SI : SDV_ENC_FMT_PCM16X0_EI;
        d.header_lines = pcm1 ? 1 : 0;
        d.black = 30; d.white = 200; d.width = 720; d.data_start = 4; d.data_stop = 716;
        bool from44100 = false, preemph = false;
        for (int i = 5; i < argc; i++) {
            const std::string opt = argv[i];
            if (opt == "bff") d.field_order = SDV_ENC_BFF;
            else if (opt == "emphasis" && !pcm1) d.ctrl_flags |= SDV_ENC_ML_EMPHASIS;
            else if (opt == "44100" && !pcm1) d.ctrl_flags |= SDV_ENC_ML_RATE_44100;
            else if (opt == "from44100") from44100 = true;
            else if (opt == "preemph") { preemph = true; if (!pcm1) d.ctrl_flags |= SDV_ENC_ML_EMPHASIS; }
            else if (encode_pix_fmt(opt) > 0) d.out_fmt[0] = (uint8_t)encode_pix_fmt(opt);
            else { fprintf(stderr, "usage: see the header of examples/decode_tape.cpp\n"); return 1; }
        }
        if (from44100 && (d.ctrl_flags & SDV_ENC_ML_RATE_44100)) { fprintf(stderr, "usage: from44100 is for a tape that runs at 44 056 Hz (see the header of examples/decode_tape.cpp)\n"); return 1; }
        size_t per_frame = 0, row_bytes = 0; int lines_per_field = 0;
        d.height = 2;                       /* (any: the geometry tells the lines of a field, the height follows from them) */
        const int grc = sdv_encode_markerless_geometry(&d, &per_frame, &lines_per_field, &row_bytes);
        if (grc != SDV_OK) { fprintf(stderr, "sdv_encode_markerless_geometry = %d: %s\n", grc, sdv_last_error(NULL)); return 3; }
        d.height = 2 * lines_per_field;
        size_t data_at = 0, n_in = 0;
        if (!read_wav(argv[2], in, &data_at, &n_in)) return 1;
        int16_t *d_pcm = NULL; uint8_t *d_luma = NULL;
        HIP_OK(hipMalloc((void **)&d_pcm, n_in * 4 + 4));
        HIP_OK(hipMemcpy(d_pcm, in.data() + data_at, n_in * 4, hipMemcpyHostToDevice));
        { const int crc = condition_pcm(eng, &d_pcm, &n_in, from44100, preemph, (d.ctrl_flags & SDV_ENC_ML_RATE_44100) ? 44100 : 44056); if (crc) return crc; }
        const int n = n_in ? (int)((n_in + per_frame - 1) / per_frame) : 1;     /* (no delay to play out: a frame is made from its own pairs) */
        const size_t frame_bytes = row_bytes * (size_t)d.height;       /* rows of row_bytes, no padding */
        HIP_OK(hipMalloc((void **)&d_luma, frame_bytes * n));
        SDV_OKAY(sdv_encode_markerless_frames(eng, &d, d_pcm, n_in, n, d_luma, row_bytes, frame_bytes, NULL));
        HIP_OK(hipDeviceSynchronize());
        rc = download(d_luma, frame_bytes * n, argv[3]);
        printf("%d %d %d %zu\n", n, d.width, d.height, row_bytes);
        (void)hipFree(d_pcm); (void)hipFree(d_luma);
    } else if (mode == "encode" && argc >= 4) {
        sdv_encode_desc d; memset(&d, 0, sizeof(d));
        d.ctrl_block = 1; d.black = 30; d.white = 200; d.width = 720; d.data_start = 12; d.data_stop = 708;
        bool from44100 = false, preemph = false;
        for (int i = 4; i < argc; i++) {
            const std::string opt = argv[i];
            if (opt == "pal") d.video_standard = SDV_ENC_PAL;
            else if (opt == "16") d.resolution = SDV_ENC_16BIT;
            else if (opt == "noctrl") d.ctrl_block = 0;
            else if (opt == "emphasis") d.ctrl_flags |= SDV_ENC_CTRL_EMPHASIS;
            else if (opt == "nocopy") d.ctrl_flags |= SDV_ENC_CTRL_COPY_PROHIBITED;
            else if (opt == "from44100") from44100 = true;
            else if (opt == "preemph") { preemph = true; d.ctrl_flags |= SDV_ENC_CTRL_EMPHASIS; }
            else if (encode_pix_fmt(opt) > 0) d.out_fmt[0] = (uint8_t)encode_pix_fmt(opt);
            else { fprintf(stderr, "usage: see the header of examples/decode_tape.cpp\n"); return 1; }
        }
        if (from44100 && d.video_standard == SDV_ENC_PAL) { fprintf(stderr, "usage: from44100 is for a tape that runs at 44 056 Hz (see the header of examples/decode_tape.cpp)\n"); return 1; }
        size_t per_frame = 0, row_bytes = 0; int lines_per_field = 0;
        d.height = 2;                       /* (any: the geometry tells the lines of a field, the height follows from them) */
        const int grc = sdv_encode_geometry(&d, &per_frame, &lines_per_field, &row_bytes);
        if (grc != SDV_OK) { fprintf(stderr, "sdv_encode_geometry = %d: %s\n", grc, sdv_last_error(NULL)); return 3; }
        d.height = 2 * lines_per_field;
        size_t data_at = 0, n_in = 0;
        if (!read_wav(argv[2], in, &data_at, &n_in)) return 1;
        int16_t *d_pcm = NULL; uint8_t *d_luma = NULL;
        HIP_OK(hipMalloc((void **)&d_pcm, n_in * 4 + 4));
        HIP_OK(hipMemcpy(d_pcm, in.data() + data_at, n_in * 4, hipMemcpyHostToDevice));
        { const int crc = condition_pcm(eng, &d_pcm, &n_in, from44100, preemph, d.video_standard == SDV_ENC_PAL ? 44100 : 44056); if (crc) return crc; }
        const int n = (int)((n_in + per_frame - 1) / per_frame) + 1;          /* ... and the frame that plays the delay out */
        const size_t frame_bytes = row_bytes * (size_t)d.height;       /* rows of row_bytes, no padding */
        HIP_OK(hipMalloc((void **)&d_luma, frame_bytes * n));
        SDV_OKAY(sdv_encode_frames(eng, &d, d_pcm, n_in, n, d_luma, row_bytes, frame_bytes, NULL));
        HIP_OK(hipDeviceSynchronize());
        rc = download(d_luma, frame_bytes * n, argv[3]);
        printf("%d %d %d %zu\n", n, d.width, d.height, row_bytes);
        (void)hipFree(d_pcm); (void)hipFree(d_luma);
    } else { fprintf(stderr, "usage: see the header of examples/decode_tape.cpp\n"); rc = 1; }
    if (d_pairs) (void)hipFree(d_pairs);
    sdv_engine_destroy(eng);
    return rc;
}
