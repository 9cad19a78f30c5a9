/*
 * rt_shim_check.cpp - TEST ONLY: what the host engines rely on in namespace rt (sdvpcmdecoder_amd/csrc/runtime.inc), in its emulator form, without an
 * engine and without a device.  A stand-alone program (tests/test_rt_shim.py builds it with -fsanitize=address,undefined and runs it); it prints what
 * it found wrong and returns the number of failed expectations.
 */
#define SDV_EMU 1
#include "hip_emu.h"
#include "../../sdvpcmdecoder_amd/csrc/runtime.inc"

#include <cstdio>
#include <vector>

static int failures = 0;
static const char *current = "";
static void expect(bool ok, const char *what) { if (!ok) { failures++; printf("FAILED %s: %s\n", current, what); } }

static void buffers()
{
    current = "Buf";
    rt::DevBuf<uint32_t> a;
    expect(a.p == NULL && a.cap == 0, "starts empty");
    expect(a.reserve(10, 16) == rt::OK && a.p != NULL && a.cap == 16, "reserve(10, 16) asks for 16");
    uint32_t *const first = a.p;
    a.p[15] = 7;                                    /* (the sanitizer checks that 16 elements are there) */
    expect(a.reserve(12) == rt::OK && a.p == first && a.cap == 16, "a request that fits changes nothing");
    expect(a.reserve(20, 4) == rt::OK && a.cap == 20, "alloc_n below n counts as n");
    rt::fail_alloc_in = 1;
    expect(a.reserve(100) != rt::OK, "the armed allocation fails");
    expect(a.p == NULL && a.cap == 0, "after a failure p == NULL and cap == 0 go together");
    expect(rt::fail_alloc_in == 0, "the failure is spent");
    rt::PinBuf<uint8_t> x, y;
    expect(x.reserve(3) == rt::OK && y.reserve(5) == rt::OK, "two buffers");
    uint8_t *const xp = x.p, *const yp = y.p;
    x.swap(y);
    expect(x.p == yp && x.cap == 5 && y.p == xp && y.cap == 3, "swap exchanges pointer and capacity");

    current = "reserve_all";
    rt::DevBuf<int> b0, b1, b2, b3;
    expect(b3.reserve(2) == rt::OK, "the last buffer holds two elements");
    int *const b3p = b3.p;
    rt::fail_alloc_in = 2;
    expect(rt::reserve_all(8, 8, b0, b1, b2, b3) != rt::OK, "the second allocation fails");
    expect(b0.cap == 8 && b0.p != NULL, "the buffer ahead of the failure grew");
    expect(b1.cap == 0 && b1.p == NULL, "the buffer that failed is empty");
    expect(b2.cap == 0 && b2.p == NULL && b3.cap == 2 && b3.p == b3p, "the buffers behind the failure are untouched");
    expect(rt::reserve_all(8, 12, b0, b1, b2, b3) == rt::OK && b0.cap == 8 && b1.cap == 12 && b2.cap == 12 && b3.cap == 12, "all of them, by one rule");
}

static void launch_sizes()
{
    current = "stride_steps";
    const uint32_t cases[][3] = {       /* threads, rows, slots */
        { 320, 486, 46 }, { 320, 64, 1 }, { 320, 7, 3 }, { 5, 10, 9 }, { 1, 1, 1 }, { 320, 2, 5 }, { 1000, 3, 7 }, { 2048 * 256, 486, 46 }, { 2048 * 256, 1, 1 },
        { 256, 32768, 2049 }, { 524288, 640, 2049 }, { 45, 486, 46 }, { 46, 486, 46 }, { 47, 486, 46 },
    };
    for (const auto &c : cases) {
        const rt::StrideSteps st = rt::stride_steps(c[0], c[1], c[2]);
        const uint64_t sum = (uint64_t)st.step_f * c[1] * c[2] + (uint64_t)st.step_r * c[2] + (uint64_t)st.step_c;
        if (sum != c[0] || st.step_c < 0 || (uint32_t)st.step_c >= c[2] || st.step_r < 0 || (uint32_t)st.step_r >= c[1] || st.step_f < 0) {
            failures++;
            printf("FAILED stride_steps(%u, %u, %u) = (%d, %d, %d)\n", c[0], c[1], c[2], st.step_f, st.step_r, st.step_c);
        }
    }
    current = "launch sizes";
    expect(rt::grid_stride_threads(1) == 320 && rt::grid_stride_threads((uint64_t)1 << 40) == 320, "the emulator's 320 threads");
    expect(rt::STC_LINES_MAX_GRID == 64, "the emulator's grid cap of sdv_k_stc007_lines");
    expect(rt::resident_waves(launch_sizes, 0) == 2, "the emulator's two resident waves");
    expect(!rt::CONCURRENT, "nothing runs beside the caller's stream");
}

struct WaveArgs { int tag; int *lanes; int *order; int *n_order; int *tags; };
static WaveArgs *g_callers_args = NULL;
static void k_wave(WaveArgs a)
{
    a.lanes[blockIdx.x]++;
    if (threadIdx.x == 0) {
        a.order[(*a.n_order)++] = (int)blockIdx.x;
        a.tags[blockIdx.x] = a.tag;
        if (blockIdx.x == 0) g_callers_args->tag = 99;      /* the caller's struct changes while the launch runs */
    }
}

static void wave_launch()
{
    current = "launch_waves";
    int lanes[4] = { 0, 0, 0, 0 }, order[4] = { -1, -1, -1, -1 }, n_order = 0, tags[4] = { 0, 0, 0, 0 };
    WaveArgs a = { 7, lanes, order, &n_order, tags };
    g_callers_args = &a;
    expect(rt::launch_waves(k_wave, 0, 1, a, NULL) == rt::OK && n_order == 0 && a.tag == 7, "grid 0 runs nothing");
    expect(rt::launch_waves(k_wave, 3, 1, a, NULL) == rt::OK, "grid 3");
    expect(n_order == 3 && order[0] == 0 && order[1] == 1 && order[2] == 2, "workgroups 0, 1, 2 in order");
    expect(lanes[0] == 64 && lanes[1] == 64 && lanes[2] == 64 && lanes[3] == 0, "64 lanes each");
    expect(a.tag == 99 && tags[0] == 7 && tags[1] == 7 && tags[2] == 7, "the arguments were captured by value");
    n_order = 0; lanes[0] = lanes[1] = 0; a.tag = 7;
    expect(rt::launch_waves(k_wave, 2, 5, a, NULL) == rt::OK && n_order == 2 && lanes[0] == 64 && lanes[1] == 64, "a kernel of five waves runs as one (its workers inline)");
}

struct ItemArgs { std::vector<long> *seen; };
static void item_body(const ItemArgs &a, long i) { a.seen->push_back(i); }
static void row_body(const ItemArgs &a, size_t row, unsigned i) { a.seen->push_back((long)row * 1000 + (long)i); }

static void item_launch()
{
    current = "RT_LAUNCH_ITEMS";
    std::vector<long> seen;
    ItemArgs a = { &seen };
    /* the product's wrapper of such a kernel takes thread t of ceil(n / block) * block as item first + t and leaves out t >= n */
    expect(RT_LAUNCH_ITEMS(k_none, item_body, 3, 5, 256, NULL, a) == rt::OK && seen == std::vector<long>({ 3, 4, 5, 6, 7 }), "items first .. first + n - 1, each once, in order");
    seen.clear();
    expect(RT_LAUNCH_ITEMS(k_none, item_body, 3, 0, 256, NULL, a) == rt::OK && seen.empty(), "no items: nothing");
    expect(RT_LAUNCH_ITEMS(k_none, item_body, 3, -2, 256, NULL, a) == rt::OK && seen.empty(), "a negative count: nothing");
    expect(RT_LAUNCH_ITEMS(k_none, item_body, 0u, (uint64_t)300, 256, NULL, a, 1, 2) == rt::OK && seen.size() == 300 && seen.front() == 0 && seen.back() == 299,
           "more items than a workgroup holds; further arguments of the wrapper are not the body's");
    seen.clear();
    current = "RT_LAUNCH_ROWS";
    expect(RT_LAUNCH_ROWS(k_none, row_body, (size_t)2, 3u, 256, NULL, a) == rt::OK && seen == std::vector<long>({ 0, 1, 2, 1000, 1001, 1002 }), "every item of every row");
    seen.clear();
    expect(RT_LAUNCH_ROWS(k_none, row_body, (size_t)0, 3u, 256, NULL, a) == rt::OK && seen.empty(), "no rows: nothing");
}

static void events_and_streams()
{
    current = "events";
    rt::fail_alloc_in = 1000;
    {
        rt::Event ev, timed(true);
        rt::Timer tm;
        rt::SideStreams side;
        float ms = -1.f;
        expect(rt::record(ev, NULL) == rt::OK && rt::wait(NULL, ev) == rt::OK && rt::wait_host(ev) == rt::OK && rt::record(timed, NULL) == rt::OK, "record, wait, wait_host");
        expect(tm.start(NULL) == rt::OK && tm.stop(NULL) == rt::OK && tm.elapsed_ms(&ms) == rt::OK && ms == 0.f, "a timer reports 0 ms");
        expect(side.open() && side.stream == NULL && side.mid == NULL && side.tail == NULL, "the side streams are the default stream");
        expect(rt::record(side.done[rt::SIDE_EVENTS - 1], side.stream) == rt::OK && rt::wait(side.tail, side.chosen[0]) == rt::OK && rt::wait(NULL, side.joined) == rt::OK, "the side streams' events");
        expect(rt::ssync(side.mid) == rt::OK, "ssync");
    }
    expect(rt::fail_alloc_in == 1000, "events and streams are not allocations");
    rt::fail_alloc_in = 0;
}

int main()
{
    buffers();
    launch_sizes();
    wave_launch();
    item_launch();
    events_and_streams();
    if (!failures) printf("RT_SHIM_OK\n");
    return failures;
}
