// encode_store_probe.hip - what the memory side of an MI355X takes of the store patterns a packed raster can have (profiles/encode_notes.md, "The store
// pattern"): 14.0 GB written with 16-byte stores by 2048 x 256 threads with a grid stride, nothing else in the loop; median of 10 runs between HIP
// events after 3 of warm-up, a hipMemsetAsync of the same bytes first.  Every store lies inside the buffer: a pattern permutes the 16-byte pieces
// of units * NB bytes, units a multiple of 256.
// build and run: hipcc --offload-arch=gfx950 -O3 -o encode_store_probe tools/encode_store_probe.hip && ./encode_store_probe
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
#include <algorithm>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)
// MODE 0: lane owns NB contiguous bytes (NB/16 stores, lane stride NB).  MODE 1: quad interleave: 4 lanes own 4 NB bytes, store k of lane q is piece q + 4 k.
// MODE 2: fully coalesced: a wave owns 64 NB bytes, store k of lane l is piece l + 64 k.
template <int NB, int MODE> __global__ void __launch_bounds__(256) k_store(uint8_t *dst, size_t units, uint32_t v)
{
    const size_t threads = (size_t)gridDim.x * 256;
    for (size_t u = (size_t)blockIdx.x * 256 + threadIdx.x; u < units; u += threads) {
        uint4 x; x.x = v ^ (uint32_t)u; x.y = v + 1; x.z = v + 2; x.w = v + 3;
        constexpr int K = NB / 16;
#pragma unroll
        for (int k = 0; k < K; k++) {
            size_t piece;
            if (MODE == 0) piece = u * K + k;
            else if (MODE == 1) piece = (u / 4) * (4 * K) + (u % 4) + 4 * k;
            else piece = (u / 64) * (64 * K) + (u % 64) + 64 * k;
            *reinterpret_cast<uint4 *>(dst + 16 * piece) = x;
        }
    }
}
template <int NB, int MODE> static int run(uint8_t *dst, size_t bytes, const char *name)
{
    const size_t units = bytes / NB / 256 * 256;     // (whole waves: every pattern stays inside units * NB bytes)
    hipEvent_t a, b; CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
    std::vector<float> t;
    for (int i = 0; i < 13; i++) {
        CK(hipEventRecord(a, 0));
        k_store<NB, MODE><<<2048, 256>>>(dst, units, (uint32_t)i);
        CK(hipEventRecord(b, 0)); CK(hipEventSynchronize(b));
        float ms; CK(hipEventElapsedTime(&ms, a, b));
        if (i >= 3) t.push_back(ms);
    }
    std::sort(t.begin(), t.end());
    printf("%-28s %8.3f ms  %6.0f GB/s\n", name, t[t.size() / 2], units * NB / t[t.size() / 2] / 1e6);
    return 0;
}
int main()
{
    const size_t bytes = 13996800000ull;
    uint8_t *dst; CK(hipMalloc((void **)&dst, bytes + 4096));
    std::vector<float> t;
    hipEvent_t a, b; CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
    for (int i = 0; i < 13; i++) { CK(hipEventRecord(a, 0)); CK(hipMemsetAsync(dst, 30, bytes, 0)); CK(hipEventRecord(b, 0)); CK(hipEventSynchronize(b)); float ms; CK(hipEventElapsedTime(&ms, a, b)); if (i >= 3) t.push_back(ms); }
    std::sort(t.begin(), t.end());
    printf("%-28s %8.3f ms  %6.0f GB/s\n", "memset", t[5], bytes / t[5] / 1e6);
    if (run<64, 0>(dst, bytes, "64 B a lane, contiguous")) return 1;
    if (run<64, 1>(dst, bytes, "64 B a lane, quad interleave")) return 1;
    if (run<64, 2>(dst, bytes, "64 B a lane, wave interleave")) return 1;
    if (run<48, 0>(dst, bytes, "48 B a lane, contiguous")) return 1;
    if (run<48, 1>(dst, bytes, "48 B a lane, quad interleave")) return 1;
    if (run<48, 2>(dst, bytes, "48 B a lane, wave interleave")) return 1;
    if (run<32, 0>(dst, bytes, "32 B a lane, contiguous")) return 1;
    if (run<32, 1>(dst, bytes, "32 B a lane, quad interleave")) return 1;
    if (run<32, 2>(dst, bytes, "32 B a lane, wave interleave")) return 1;
    if (run<16, 0>(dst, bytes, "16 B a lane")) return 1;
    CK(hipFree(dst));
    return 0;
}
