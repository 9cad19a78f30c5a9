/*
 * runtime.inc - namespace rt: everything the host engines ask of the runtime, once for each of the two builds.
 *
 * Included by engine.inc ahead of everything that uses it.  The product (sdvpcm_hip.hip) gets the HIP runtime: memory, copies, kernel launches,
 * events and streams.  The tests' build (tests/emu/emu_engine.cpp, -DSDV_EMU) gets malloc / memcpy, the SIMT emulator's launch (emu::launch) and
 * events and streams that do nothing: everything there runs in order, at once.  The two variants of a thing stand side by side here and nowhere
 * else - the engines (*.inc) are the same code in both builds, without a conditional and without a call of the runtime's own.
 *
 * Kernels are launched in one of two ways:
 *   rt::launch_waves / RT_LAUNCH64     wave kernels: a workgroup is k waves of 64 lanes working together, a workgroup per unit of work
 *   RT_LAUNCH_ITEMS / RT_LAUNCH_ROWS   thread-per-item kernels: item i is body(args, i); the product launches the __global__ wrapper around the body
 */
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>

namespace rt {
#ifndef SDV_EMU
/* ---- the product: HIP ------------------------------------------------------------------------------------------------------------ */
typedef hipStream_t stream_t;
typedef hipError_t status_t;
static const status_t OK = hipSuccess;
static const bool CONCURRENT = true;            /* streams run beside each other: work may be queued on side streams (SideStreams) */
static inline const char *err_str(status_t e) { return hipGetErrorString(e); }
#ifndef SDV_DEV_AIDS
static inline status_t dmalloc(void **p, size_t n) { return hipMalloc(p, n); }
static inline status_t hpin(void **p, size_t n) { return hipHostMalloc(p, n, hipHostMallocDefault); }      /* page-locked host memory: copies into it are asynchronous */
#else
/* Developer builds (tests): with SDV_POISON_ALLOC=<byte> in the environment every new allocation is filled with that byte before it is handed out, so
 * that what a kernel reads before anything wrote it is not the zero a young process usually finds there (tests/test_memory_history.py).  Unset:
 * nothing is filled.  sdv_dev_poisoned counts what was filled since the library was loaded. */
static std::atomic<uint64_t> poisoned_allocs{ 0 }, poisoned_bytes{ 0 };
static inline int poison_byte() { const char *v = getenv("SDV_POISON_ALLOC"); return v && *v ? (int)(strtol(v, NULL, 0) & 0xFF) : -1; }
static inline void poisoned(size_t n) { poisoned_allocs++; poisoned_bytes += n; }
static inline status_t dmalloc(void **p, size_t n)
{
    status_t st = hipMalloc(p, n);
    const int b = poison_byte();
    if (st != OK || b < 0 || n == 0) return st;
    st = hipMemset(*p, b, n);
    if (st == OK) st = hipDeviceSynchronize();          /* (the fill is there before any stream of the engine touches the memory) */
    if (st != OK) { (void)hipFree(*p); *p = NULL; return st; }
    poisoned(n);
    return OK;
}
static inline status_t hpin(void **p, size_t n)
{
    const status_t st = hipHostMalloc(p, n, hipHostMallocDefault);
    const int b = poison_byte();
    if (st == OK && b >= 0 && n > 0) { memset(*p, b, n); poisoned(n); }
    return st;
}
#endif
static inline status_t dfree(void *p) { return hipFree(p); }
static inline status_t hunpin(void *p) { return hipHostFree(p); }
static inline status_t ssync(stream_t s) { return hipStreamSynchronize(s); }
static inline status_t h2d(void *d, const void *h, size_t n, stream_t s) { return hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, s); }
static inline status_t d2d(void *d, const void *s_, size_t n, stream_t s) { return hipMemcpyAsync(d, s_, n, hipMemcpyDeviceToDevice, s); }
static inline status_t dfill_bytes(void *p, int v, size_t n, stream_t s) { return hipMemsetAsync(p, v, n, s); }
/* read-back that is only queued: h is page-locked (rt::hpin) and is read after rt::ssync or rt::wait_host */
static inline status_t d2h_async(void *h, const void *d, size_t n, stream_t s) { return hipMemcpyAsync(h, d, n, hipMemcpyDeviceToHost, s); }
/* ... and waited for */
static inline status_t d2h_pinned(void *h, const void *d, size_t n, stream_t s) { const status_t e = d2h_async(h, d, n, s); return e != OK ? e : ssync(s); }
/* Synchronous read-back.  A copy into pageable memory costs ~35 us whatever its size (the runtime stages it); the counts, flags and states
 * the schedulers read several times per call go through a page-locked bounce buffer instead (~12 us) - one per host thread that ever reads
 * back (engines of different threads do not wait for each other), 1 MB, kept for the life of the process. */
enum { BOUNCE_BYTES = 1 << 20 };
/* The buffer belongs to the engine whose entry point is running on this thread (SDV_ON_DEVICE names it; allocated on first use under that engine's
 * device, freed with the engine): host programs that call from short-lived threads leave nothing pinned behind. */
struct BounceSlot { void *p = NULL; bool tried = false; ~BounceSlot() { if (p) (void)hunpin(p); } };
static thread_local BounceSlot *tls_bounce_slot = NULL;
struct BounceScope {
    BounceSlot *prev;
    explicit BounceScope(BounceSlot *slot) : prev(tls_bounce_slot) { tls_bounce_slot = slot; }
    ~BounceScope() { tls_bounce_slot = prev; }
};
static inline void *bounce()
{
    BounceSlot *b = tls_bounce_slot;
    if (!b) return NULL;
    if (!b->p && !b->tried) { b->tried = true; if (hpin(&b->p, BOUNCE_BYTES) != OK) { b->p = NULL; (void)hipGetLastError(); } }
    return b->p;
}
static inline status_t d2h(void *h, const void *d, size_t n, stream_t s)
{
    void *b = n > 0 && n <= (size_t)BOUNCE_BYTES ? bounce() : NULL;
    if (!b) return d2h_pinned(h, d, n, s);
    const status_t e = d2h_pinned(b, d, n, s); if (e != OK) return e;
    memcpy(h, b, n);
    return OK;
}
/* Every entry point runs on its engine's device and leaves the caller's current device as it found it. */
struct DeviceGuard {
    int prev; bool switched; status_t err;
    explicit DeviceGuard(int device) : prev(-1), switched(false), err(OK)
    {
        err = hipGetDevice(&prev);
        if (err == OK && prev != device) { err = hipSetDevice(device); switched = err == OK; }
    }
    ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
    status_t status() const { return err; }
};

/* Wave kernels: `grid` workgroups of `waves` x 64 lanes (grid 0: nothing). */
template <class K, class A> static inline status_t launch_waves(K kernel, size_t grid, unsigned waves, const A &a, stream_t s)
{
    if (grid == 0) return OK;
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(64 * waves), 0, s, a);
    return hipGetLastError();
}
/* Thread-per-item kernels: the __global__ wrapper `kernel` over the workgroups of `block` threads that hold n items, `rows` times (grid.y); what comes
 * after the stream are the wrapper's arguments.  The wrapper finds the item of a thread (first + its index) and leaves out those past the last.
 * The emulator runs `body` instead: body(args, first + i) for i in [0, n), and body(args, row, i) for every row of RT_LAUNCH_ROWS. */
template <class K, class N, class... A> static inline status_t launch_threads(K kernel, N n, size_t rows, unsigned block, stream_t s, const A &...a)
{
    if (!(n > 0) || rows == 0) return OK;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((n + (block - 1)) / block), (unsigned)rows), dim3(block), 0, s, a...);
    return hipGetLastError();
}
#define RT_LAUNCH_ITEMS(kernel, body, first, n, block, stream, ...) rt::launch_threads(kernel, n, 1, block, stream, __VA_ARGS__)
#define RT_LAUNCH_ROWS(kernel, body, rows, n, block, stream, ...) rt::launch_threads(kernel, n, rows, block, stream, __VA_ARGS__)

/* launch sizes that are the build's own */
enum : unsigned { STC_LINES_MAX_GRID = 65536 };         /* sdv_k_stc007_lines: a wave takes the lines a grid apart */
/* threads of a launch whose grid stride walks the rest (sdv_k_ingest, sdv_k_encode_raster): workgroups of 256, at most 2048 of them - every CU of the
 * MI355X eight times over.  A thread takes a second trip only in a call of more than 2048 x 256 items. */
static inline uint32_t grid_stride_threads(uint64_t items) { const uint64_t wg = (items + 255) / 256; return 256u * (uint32_t)(wg < 2048 ? wg : 2048); }
/* waves of a one-wave kernel the device holds at once (they share their work through a queue) */
template <class K> static inline size_t resident_waves(K kernel, int device)
{
    int per_cu = 0, cus = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 64, 0) != hipSuccess || per_cu <= 0) per_cu = 8;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) cus = 256;
    const size_t waves = (size_t)per_cu * (size_t)cus;
    return waves > 8192 ? 8192 : waves;
}

/* An event, made when it is first recorded (or by create()); destroyed with its owner, under the owner's device (like Buf).  timed: rt::Timer's. */
struct Event {
    hipEvent_t ev = NULL; const bool timed;
    explicit Event(bool timed_ = false) : timed(timed_) {}
    Event(const Event &) = delete;
    Event &operator=(const Event &) = delete;
    ~Event() { if (ev) (void)hipEventDestroy(ev); }
    status_t create()
    {
        if (ev) return OK;
        const status_t st = timed ? hipEventCreate(&ev) : hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        if (st != OK) ev = NULL;
        return st;
    }
};
static inline status_t record(Event &e, stream_t s) { const status_t st = e.create(); return st != OK ? st : hipEventRecord(e.ev, s); }
static inline status_t wait(stream_t s, Event &e) { return e.ev ? hipStreamWaitEvent(s, e.ev, 0) : OK; }       /* (never recorded: nothing to wait for) */
static inline status_t wait_host(Event &e) { return e.ev ? hipEventSynchronize(e.ev) : OK; }
/* device time between two points of a stream (sdv_set_profiling) */
struct Timer {
    Event t0{ true }, t1{ true };
    status_t start(stream_t s) { return record(t0, s); }
    status_t stop(stream_t s) { return record(t1, s); }
    status_t elapsed_ms(float *ms) { const status_t st = wait_host(t1); return st != OK ? st : hipEventElapsedTime(ms, t0.ev, t1.ev); }     /* waits for stop() */
};
/* Three streams beside the caller's and the events that order work between them (the batches of sdv_pcm16x0_stitch_frames). */
enum { SIDE_EVENTS = 64 };
struct SideStreams {
    stream_t stream, mid, tail; bool ok = false;
    Event start, joined, done[SIDE_EVENTS], chosen[SIDE_EVENTS], decided[SIDE_EVENTS];
    bool open()         /* made on first use; false: go without */
    {
        if (ok) return true;
        if (hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != OK || hipStreamCreateWithFlags(&tail, hipStreamNonBlocking) != OK ||
            hipStreamCreateWithFlags(&mid, hipStreamNonBlocking) != OK) return false;
        if (start.create() != OK || joined.create() != OK) return false;
        for (int i = 0; i < SIDE_EVENTS; i++) if (done[i].create() != OK || decided[i].create() != OK || chosen[i].create() != OK) return false;
        return ok = true;
    }
    /* waits for the side streams: an owner declares it behind the buffers their kernels use, so that it goes first */
    ~SideStreams()
    {
        if (!ok) return;
        (void)ssync(stream); (void)ssync(mid); (void)ssync(tail);
        (void)hipStreamDestroy(stream); (void)hipStreamDestroy(mid); (void)hipStreamDestroy(tail);
    }
};

#else
/* ---- the tests' build: host memory and the SIMT emulator --------------------------------------------------------------------------- */
typedef void *stream_t;
typedef int status_t;
static const status_t OK = 0;
static const bool CONCURRENT = false;           /* everything runs where it is queued, at once */
static inline const char *err_str(status_t) { return "the emulated runtime refused"; }
/* (tests: the fail_alloc_in-th allocation from now fails, once - sdv_emu_fail_alloc, tests/emu/emu_engine.cpp) */
static int fail_alloc_in = 0;
/* (tests: every allocation that succeeds is filled with this byte; negative: left as malloc gives it - sdv_emu_poison_alloc, tests/emu/emu_engine.cpp) */
static int poison_alloc = -1;
static inline status_t emu_alloc(void **p, size_t n)
{
    if (fail_alloc_in > 0 && --fail_alloc_in == 0) { *p = NULL; return 1; }
    *p = malloc(n ? n : 1);
    if (*p && poison_alloc >= 0) memset(*p, poison_alloc, n ? n : 1);
    return *p ? 0 : 1;
}
static inline status_t dmalloc(void **p, size_t n) { return emu_alloc(p, n); }
static inline status_t dfree(void *p) { free(p); return OK; }
static inline status_t hpin(void **p, size_t n) { return emu_alloc(p, n); }
static inline status_t hunpin(void *p) { free(p); return OK; }
static inline status_t ssync(stream_t) { return OK; }
static inline status_t h2d(void *d, const void *h, size_t n, stream_t) { memcpy(d, h, n); return OK; }
static inline status_t d2d(void *d, const void *s_, size_t n, stream_t) { memcpy(d, s_, n); return OK; }
static inline status_t dfill_bytes(void *p, int v, size_t n, stream_t) { memset(p, v, n); return OK; }
static inline status_t d2h_async(void *h, const void *d, size_t n, stream_t) { memcpy(h, d, n); return OK; }
static inline status_t d2h_pinned(void *h, const void *d, size_t n, stream_t) { memcpy(h, d, n); return OK; }
static inline status_t d2h(void *h, const void *d, size_t n, stream_t) { memcpy(h, d, n); return OK; }
struct BounceSlot {};
struct BounceScope { explicit BounceScope(BounceSlot *) {} };
struct DeviceGuard {
    explicit DeviceGuard(int) {}
    status_t status() const { return OK; }
};

/* Wave kernels: the workgroups one after the other, 64 lanes each (a kernel of several waves runs its workers inline); the arguments are captured by value. */
template <class K, class A> static inline status_t launch_waves(K kernel, size_t grid, unsigned, const A &a, stream_t)
{
    if (grid > 0) emu::launch((unsigned)grid, [kernel, a]() { kernel(a); });
    return OK;
}
/* Thread-per-item kernels: the body over the items, in order (the product's form above says what the arguments mean). */
template <class A, class... R> static inline const A &first_arg(const A &a, const R &...) { return a; }
template <class I, class N, class F> static inline status_t each_item(I first, N n, F f) { for (N i = 0; i < n; i++) f((N)((N)first + i)); return OK; }
template <class N, class F> static inline status_t each_row_item(size_t rows, N n, F f) { for (size_t r = 0; r < rows; r++) for (N i = 0; i < n; i++) f(r, i); return OK; }
#define RT_LAUNCH_ITEMS(kernel, body, first, n, block, stream, ...) rt::each_item(first, n, [&](auto i_) { body(rt::first_arg(__VA_ARGS__), i_); })
#define RT_LAUNCH_ROWS(kernel, body, rows, n, block, stream, ...) rt::each_row_item(rows, n, [&](size_t r_, auto i_) { body(rt::first_arg(__VA_ARGS__), r_, i_); })

/* Few threads and small grids: every test walks the grid strides of the kernels, with carries from slots to rows to frames. */
enum : unsigned { STC_LINES_MAX_GRID = 64 };
static inline uint32_t grid_stride_threads(uint64_t) { return 320; }
template <class K> static inline size_t resident_waves(K, int) { return 2; }

struct Event { explicit Event(bool = false) {} };
static inline status_t record(Event &, stream_t) { return OK; }
static inline status_t wait(stream_t, Event &) { return OK; }
static inline status_t wait_host(Event &) { return OK; }
struct Timer {
    status_t start(stream_t) { return OK; }
    status_t stop(stream_t) { return OK; }
    status_t elapsed_ms(float *ms) { *ms = 0.f; return OK; }
};
enum { SIDE_EVENTS = 64 };
struct SideStreams {
    stream_t stream = NULL, mid = NULL, tail = NULL;
    Event start, joined, done[SIDE_EVENTS], chosen[SIDE_EVENTS], decided[SIDE_EVENTS];
    bool open() { return true; }
};
#endif

/* ---- both builds ------------------------------------------------------------------------------------------------------------------- */
#define RT_CHECK(expr) do { rt::status_t _e = (expr); if (_e != rt::OK) { set_error(e, std::string(#expr) + ": " + rt::err_str(_e)); return SDV_ERR_HIP; } } while (0)
/* a one-wave kernel, a workgroup per unit of work, from a function that returns an SDV_ code */
#define RT_LAUNCH64(kernel, grid, args, stream) RT_CHECK(rt::launch_waves(kernel, grid, 1, args, stream))
#define SDV_ON_DEVICE(e) rt::DeviceGuard device_guard_((e)->device); RT_CHECK(device_guard_.status()); rt::BounceScope bounce_scope_(&(e)->bounce)

/* A launch of `threads` threads over frames of `rows` rows of `slots` items, a thread per item: how far the grid stride takes a thread on,
 * as whole frames, rows and slots (step_f * rows * slots + step_r * slots + step_c == threads). */
struct StrideSteps { int step_f, step_r, step_c; };
static inline StrideSteps stride_steps(uint32_t threads, uint32_t rows, uint32_t slots)
{
    const uint32_t lines = threads / slots;
    return { (int)(lines / rows), (int)(lines % rows), (int)(threads % slots) };
}

/* Device memory (DevBuf) and page-locked host memory (PinBuf) of the engines: grow-only, counted in elements, freed by the destructor - which must run
 * with the engine's device current (sdv_engine_destroy).  reserve(n) leaves a buffer of at least n elements whose old contents are gone; alloc_n is what
 * a growing buffer asks the runtime for (the call site's growth rule).  After a failure the buffer is empty: p == NULL and cap == 0 always go together. */
struct DevMem { static status_t get(void **p, size_t bytes) { return dmalloc(p, bytes); } static void put(void *p) { (void)dfree(p); } };
struct PinMem { static status_t get(void **p, size_t bytes) { return hpin(p, bytes); } static void put(void *p) { (void)hunpin(p); } };
template <typename T, typename Mem> struct Buf {
    T *p = NULL; size_t cap = 0;
    Buf() = default;
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    ~Buf() { release(); }
    operator T *() const { return p; }
    void release() { if (p) Mem::put(p); p = NULL; cap = 0; }
    void swap(Buf &o) { std::swap(p, o.p); std::swap(cap, o.cap); }
    status_t reserve(size_t n, size_t alloc_n = 0)
    {
        if (n <= cap) return OK;
        if (alloc_n < n) alloc_n = n;
        release();
        const status_t st = Mem::get((void **)&p, alloc_n * sizeof(T));
        if (st != OK) { p = NULL; return st; }
        cap = alloc_n;
        return OK;
    }
};
template <typename T> using DevBuf = Buf<T, DevMem>;
template <typename T> using PinBuf = Buf<T, PinMem>;
/* buffers that grow by one rule, in one statement: the first failure ends it */
template <typename... B> static inline status_t reserve_all(size_t n, size_t alloc_n, B &...b) { status_t st = OK; (void)(((st = b.reserve(n, alloc_n)) == OK) && ...); return st; }
} // namespace rt

#if defined(SDV_DEV_AIDS) && !defined(SDV_EMU)
/* Developer builds of the HIP library (tests): what SDV_POISON_ALLOC has filled since the library was loaded ... */
extern "C" int sdv_dev_poisoned(uint64_t *allocations, uint64_t *bytes)
{
    if (allocations) *allocations = rt::poisoned_allocs.load();
    if (bytes) *bytes = rt::poisoned_bytes.load();
    return rt::poison_byte();           /* the byte in force, -1: none */
}
/* ... and what a fresh allocation of `bytes` bytes holds, device (pinned 0) or page-locked (pinned 1), through the calls the engines' buffers make: the
 * proof that the fill lands in both kinds of memory.  0, or the runtime's error. */
extern "C" int sdv_dev_peek_fresh(int pinned, size_t bytes, uint8_t *out)
{
    if (!out || bytes == 0) return -1;
    void *p = NULL;
    rt::status_t st = pinned ? rt::hpin(&p, bytes) : rt::dmalloc(&p, bytes);
    if (st != rt::OK) return (int)st;
    if (pinned) memcpy(out, p, bytes);
    else st = hipMemcpy(out, p, bytes, hipMemcpyDeviceToHost);
    (void)(pinned ? rt::hunpin(p) : rt::dfree(p));
    return (int)st;
}
#endif
