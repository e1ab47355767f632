// lzgpu_api.hip -- C ABI (include/lzgpu.h), device context and host-side orchestration of the
// seed stage.  The host work here is what the reference does around its hot loops and is not
// data-parallel: seed compilation (src/seeds.c), score-class compression of the 256x256 matrix,
// chunk planning, and the per-HSP finish (discovery ordering + the floating-point entropy
// adjustment of src/seed_search.c:2851-2874, src/dna_utilities.c:2888-2936).
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <algorithm>
#include <mutex>
#include <thread>
#include <atomic>
#include "lz_ctx.hpp"
#include "lz_host.hpp"
#include "lz_lut.hpp"
#include "lz_exact.hpp"
#include "lz_mismatch.hpp"
#include "lz_filter.hpp"

// ------------------------------------------------------------------------------ context

static LzCtx g_ctx;
void lz_phase_clocks_print();                                 // settle_kernels.hip (prints only in a -DLZ_PHASE_CLOCKS build)
LzCtx& lz_ctx() { return g_ctx; }

// The last error message: one per THREAD (B3 may run on a second host thread beside B2, and the problems of a batch run on
// threads of their own), plus the newest of any thread for a caller that had no failure of its own -- lzgpu_gapped_extend_batch
// reports a worker's failure from the calling thread.  lzgpu_last_error() hands out the calling thread's own copy: no torn reads,
// never a pointer into a string another thread may reassign.
static thread_local std::string t_last_error, t_last_error_out;
static std::mutex g_err_m;
int lz_fail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof(buf), fmt, ap); va_end(ap);
    t_last_error = buf;
    std::lock_guard<std::mutex> lk(g_err_m);
    g_ctx.last_error = buf;
    return code;
}

int DevBuf::ensure(size_t bytes)
{
    if (bytes <= cap && p) return 0;
    const bool prof = lz_settings().hostprof;
    const auto t0 = std::chrono::steady_clock::now();
    const size_t old = cap;
    if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
    const auto t1 = std::chrono::steady_clock::now();
    size_t want = bytes < 256 ? 256 : bytes;
    if (want >= (64u << 20)) {                                  // big buffers in steps of 1/16 of their size: a request that
        size_t step = (size_t)1 << 22;                          // creeps up (the second strand's chunks, a few more DPs) does
        while (step * 32 <= want) step <<= 1;                   // not free and re-allocate gigabytes
        want = (want + step - 1) / step * step;
    }
    hipError_t e = hipMalloc(&p, want);
    if (prof && want >= (64u << 20)) fprintf(stderr, "[lzgpu hostprof] device buffer %zu -> %zu MiB at %p: hipFree %.1f ms, hipMalloc %.1f ms\n", old >> 20, want >> 20, p,
                                             std::chrono::duration<double, std::milli>(t1 - t0).count(), std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count());
    if (e != hipSuccess) { p = nullptr; return lz_fail(LZGPU_ERR_OOM, "hipMalloc(%zu) failed: %s", want, hipGetErrorString(e)); }
    cap = want;
    return 0;
}
void DevBuf::release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }

int KernelTimer::id_of(const char* name)
{
    for (size_t i = 0; i < names.size(); i++) if (names[i] == name) return (int)i;
    names.push_back(name); launches.push_back(0); ms.push_back(0.0);
    return (int)names.size() - 1;
}
hipEvent_t KernelTimer::get_event(hipStream_t s)
{
    auto& pl = pool[s];
    if (!pl.empty()) { hipEvent_t e = pl.back(); pl.pop_back(); return e; }
    hipEvent_t e; (void)hipEventCreate(&e); return e;
}
void KernelTimer::begin(const char* name, hipStream_t s)
{
    if (!enabled) return;
    const std::string& only = lz_settings().timer_only;         // profiling aid: time just this kernel
    if (!only.empty() && only != name) { cur = -1; return; }
    cur = id_of(name); cur_a = get_event(s);
    (void)hipEventRecord(cur_a, s);
}
void KernelTimer::end(hipStream_t s)
{
    if (!enabled || cur < 0) return;
    hipEvent_t b = get_event(s);
    (void)hipEventRecord(b, s);
    pending.push_back({cur, cur_a, b, s});
    cur = -1; cur_a = nullptr;
}
void KernelTimer::resolve()
{
    // LZGPU_GAPS=1 (profiling aid): idle time on a stream between the end of one timed kernel and the
    // start of the next, reported when it exceeds 0.3 ms
    const bool gaps = lz_settings().gaps;
    static std::map<hipStream_t, Pending> last;
    std::vector<Pending> later;
    for (auto& p : pending) {
        float t = 0.f;
        const hipError_t e = hipEventElapsedTime(&t, p.a, p.b);
        if (e == hipErrorNotReady) { later.push_back(p); continue; }     // recorded after the last synchronisation
        if (e == hipSuccess) { ms[p.id] += t; launches[p.id]++; }
        if (gaps) {
            auto it = last.find(p.s);
            float g = 0.f;
            if (it != last.end() && hipEventElapsedTime(&g, it->second.b, p.a) == hipSuccess && g > 0.3f)
                fprintf(stderr, "[lzgpu gaps] %.2f ms idle between %s and %s\n", g, names[it->second.id].c_str(), names[p.id].c_str());
            if (it != last.end()) { pool[it->second.s].push_back(it->second.a); pool[it->second.s].push_back(it->second.b); }
            last[p.s] = p;
            continue;
        }
        pool[p.s].push_back(p.a); pool[p.s].push_back(p.b);
    }
    pending.swap(later);
}
void KernelTimer::reset() { resolve(); for (auto& x : ms) x = 0; for (auto& x : launches) x = 0; }

// HIP's current device is a property of the HOST THREAD.  The context may have been brought up on another thread
// (lzgpu_init_async's, or whichever thread called lzgpu_init first), so every entry point that touches the device
// first binds the calling thread to the library's device: without it a rank r > 0 of a multi-GPU run would allocate
// and copy on device 0 while its streams live on device r.  (hipSetDevice on the device that is already current
// is a thread-local store.)
int lz_bind_thread()
{
    if (!g_ctx.inited) { int rc = lzgpu_init(-1); if (rc) return rc; }
    LZ_HIP(hipSetDevice(g_ctx.device));
    return 0;
}
static int require_init() { return lz_bind_thread(); }

extern "C" const char* lzgpu_last_error(void)
{
    if (!t_last_error.empty()) t_last_error_out = t_last_error;
    else { std::lock_guard<std::mutex> lk(g_err_m); t_last_error_out = g_ctx.last_error; }
    return t_last_error_out.c_str();
}

extern "C" int lzgpu_probe(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return lz_fail(LZGPU_ERR_NO_DEVICE, "no HIP device visible");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, 0) != hipSuccess) return lz_fail(LZGPU_ERR_NO_DEVICE, "hipGetDeviceProperties failed");
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return lz_fail(LZGPU_ERR_NO_DEVICE, "device 0 is %s, this library is built for gfx950 only", prop.gcnArchName);
    return 0;
}

static int lz_init_locked(int device_index)
{
    if (g_ctx.inited && (device_index < 0 || device_index == g_ctx.device)) return 0;
    if (g_ctx.inited) return lz_fail(LZGPU_ERR_STATE, "already bound to device %d", g_ctx.device);
    int rc = lzgpu_probe();
    if (rc) return rc;
    if (device_index < 0) {
        const char* lr = getenv("LOCAL_RANK");
        device_index = lr ? atoi(lr) : 0;
        int n = 0; (void)hipGetDeviceCount(&n);
        if (n > 0) device_index %= n;
    }
    LZ_HIP(hipSetDevice(device_index));
    { hipDeviceProp_t prop; if (hipGetDeviceProperties(&prop, device_index) == hipSuccess && prop.multiProcessorCount > 0) g_ctx.num_cus = prop.multiProcessorCount; }
    LZ_HIP(hipStreamCreateWithFlags(&g_ctx.stream, hipStreamNonBlocking));
    LZ_HIP(hipStreamCreateWithFlags(&g_ctx.dp_stream, hipStreamNonBlocking));
    const LzSettings& S = lz_settings();                       // (the first init of the process reads them)
    if (S.scan_mode >= 0) g_ctx.min_scan_mode = S.scan_mode;
    if (S.hit_capacity) g_ctx.hit_capacity = S.hit_capacity;
    g_ctx.device = device_index;
    g_ctx.inited = true;
    return 0;
}

// lzgpu_init_async: the same on a detached thread; every path into lzgpu_init first waits for it (and so does exit():
// the runtime must not be torn down under a thread that is still bringing it up)
static std::mutex g_init_mutex;
static std::atomic<int> g_async_state{0};                      // 0: never asked, 1: running, 2: finished
static void lz_wait_async() { while (g_async_state.load(std::memory_order_acquire) == 1) std::this_thread::yield(); }
extern "C" void lzgpu_init_async(int device_index)
{
    int expect = 0;
    if (!g_async_state.compare_exchange_strong(expect, 1)) return;
    atexit(lz_wait_async);
    std::thread([device_index]() {
        { std::lock_guard<std::mutex> lk(g_init_mutex); (void)lz_init_locked(device_index); }
        g_async_state.store(2, std::memory_order_release);
    }).detach();
}
extern "C" int lzgpu_init(int device_index)
{
    lz_wait_async();
    std::lock_guard<std::mutex> lk(g_init_mutex);
    const int rc = lz_init_locked(device_index);
    if (!rc) LZ_HIP(hipSetDevice(g_ctx.device));               // the caller's thread too (the context may be another thread's work)
    return rc;
}
extern "C" int lzgpu_device_index(void) { return g_ctx.inited ? g_ctx.device : -1; }

extern "C" void lzgpu_shutdown(void)
{
    LzCtx& c = g_ctx;
    if (!c.inited) return;
    (void)hipSetDevice(c.device);
    (void)hipStreamSynchronize(c.stream);
    lz_phase_clocks_print();
    if (c.dp_stream) (void)hipStreamSynchronize(c.dp_stream);
    c.timer.resolve(); c.dp_timer.resolve();
    c.release_device_memory();                                  // (lz_ctx.hpp, beneath the members)
    (void)hipStreamDestroy(c.stream);
    if (c.dp_stream) (void)hipStreamDestroy(c.dp_stream);
    c.stream = nullptr; c.dp_stream = nullptr; c.inited = false; c.device = -1;
    c.n_owners = 1; c.owner = 0; c.last_order.clear();
    c.filter_on = false; c.filter_dropped = 0;
}

extern "C" void lzgpu_free(void* p) { free(p); }

// ------------------------------------------------------------------------------ sequences

static int slot_upload(LzCtx& c, SeqSlot& s, const u8* bytes, u32 len, bool keep_host, hipStream_t st = nullptr)
{
    int rc;
    if (!st) st = c.stream;
    size_t total = (size_t)len + 2 * LZ_SEQ_PAD + 16;
    if ((rc = s.raw.ensure(total))) return rc;
    if ((rc = s.code.ensure(total))) return rc;
    LZ_HIP(hipMemsetAsync(s.raw.p, 0, total, st));
    LZ_HIP(hipMemsetAsync(s.code.p, LZ_CODE_INVALID, total, st));
    if (len) LZ_HIP(hipMemcpyAsync(s.raw_base(), bytes, len, hipMemcpyHostToDevice, st));
    LZ_HIP(hipStreamSynchronize(st));
    s.len = len; s.have_raw = true; s.code_key = 0; s.dp_key = 0; s.match_key = 0;
    if (keep_host) s.host.assign(bytes, bytes + len); else s.host.clear();
    return 0;
}

static uint64_t fnv1a(const void* p, size_t n, uint64_t h = 1469598103934665603ull)
{
    const u8* b = (const u8*)p;
    for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 1099511628211ull; }
    return h ? h : 1;
}

// encode slot with table cls (class | bits<<5 | invalid<<7), unless already encoded with it
static int slot_encode(LzCtx& c, SeqSlot& s, const u8 cls[256], DevBuf& cls_dev)
{
    uint64_t key = fnv1a(cls, 256);
    if (s.code_key == key) return 0;
    int rc;
    if ((rc = cls_dev.ensure(256))) return rc;
    LZ_HIP(hipMemcpyAsync(cls_dev.p, cls, 256, hipMemcpyHostToDevice, c.stream));
    LZ_HIP(hipStreamSynchronize(c.stream));          // cls is caller stack memory
    if ((rc = lzk_encode(c, s.raw_base(), s.code_base(), s.len, cls_dev.as<u8>()))) return rc;
    s.code_key = key;
    // packed 4-bit codes for phase A when the matrix has fewer than 8 classes
    bool small = true;
    for (int b = 0; b < 256; b++) if ((cls[b] & 31u) >= 8u) { small = false; break; }
    s.have_nib = false;
    if (small) {
        const size_t total = (size_t)s.len + 2 * LZ_SEQ_PAD + 16;   // the code allocation (even)
        if ((rc = s.nib.ensure(total / 2 + 64))) return rc;
        LZ_HIP(hipMemsetAsync(s.nib.p, 0, total / 2 + 64, c.stream));
        if ((rc = lzk_pack_nibbles(c, s.code.as<u8>(), s.nib.as<u8>(), total / 2))) return rc;
        s.have_nib = true;
    }
    // 2-bit codes, special mask and the set of byte values that occur (phase A on look-up tables, lz_lut.hpp)
    const u32 nmask = (u32)(((size_t)s.len + 2 * LZ_PAD2 + 7) / 8 + 16);
    if ((rc = s.two.ensure((size_t)nmask * 2 + 96))) return rc;       // (+ what k_overlap32's last block reads past the end)
    if ((rc = s.spc.ensure((size_t)nmask + 96))) return rc;
    if ((rc = s.occ_dev.ensure(256 * 4))) return rc;
    LZ_HIP(hipMemsetAsync(s.two.p, 0, (size_t)nmask * 2 + 96, c.stream));
    LZ_HIP(hipMemsetAsync(s.spc.p, 0xFF, (size_t)nmask + 96, c.stream));
    if ((rc = lzk_pack2(c, s.code_base(), s.raw_base(), s.len, s.two.as<u8>(), s.spc.as<u8>(), nmask, s.occ_dev.as<u32>()))) return rc;
    if (&s == &c.target) {                                     // (the target only: k_scan_hits reads these instead of the plain arrays)
        const size_t nb2 = ((size_t)nmask * 2 + 31) / 32, nb1 = ((size_t)nmask + 31) / 32;
        if ((rc = s.two_x.ensure(nb2 * 64 + 64))) return rc;
        if ((rc = s.spc_x.ensure(nb1 * 64 + 64))) return rc;
        if ((rc = lzk_overlap32(c, s.two.as<u8>(), s.two_x.as<u8>(), nb2))) return rc;
        if ((rc = lzk_overlap32(c, s.spc.as<u8>(), s.spc_x.as<u8>(), nb1))) return rc;
    }
    u32 flags[256];
    LZ_HIP(hipMemcpyAsync(flags, s.occ_dev.p, sizeof(flags), hipMemcpyDeviceToHost, c.stream));
    LZ_HIP(hipStreamSynchronize(c.stream));
    s.has_special = false;
    for (int b = 0; b < 256; b++) { s.occ[b] = flags[b] ? 1 : 0; if (flags[b] && (cls[b] & LZ_CODE_INVALID)) s.has_special = true; }
    return 0;
}

// the match codes of slot s for an exact-match search (lz_exact.hpp), unless it holds those of the same match_bits already:
// the encode and pack passes once more with the match classes, through scratch code bytes of the slot's geometry
static int slot_match_encode(LzCtx& c, SeqSlot& s, const int8_t match_bits[256])
{
    u8 cls[256];
    lz_exact_cls(match_bits, cls);
    const uint64_t key = fnv1a(cls, 256);
    if (s.match_key == key && s.mtwo.p && s.mspc.p) return 0;
    int rc;
    s.match_key = 0;
    const size_t total = (size_t)s.len + 2 * LZ_SEQ_PAD + 16, code_at = 2048;     // scratch: class map | presence flags at 256 | code bytes at 2048
    if ((rc = c.match_tmp.ensure(code_at + total))) return rc;
    u8* const tmp = c.match_tmp.as<u8>();
    u8* const code_base = tmp + code_at + LZ_SEQ_PAD;
    LZ_HIP(hipMemcpyAsync(tmp, cls, 256, hipMemcpyHostToDevice, c.stream));
    LZ_HIP(hipMemsetAsync(tmp + code_at, LZ_CODE_INVALID, total, c.stream));
    LZ_HIP(hipStreamSynchronize(c.stream));          // cls is stack memory
    if ((rc = lzk_encode(c, s.raw_base(), code_base, s.len, tmp))) return rc;
    const u32 nmask = (u32)(((size_t)s.len + 2 * LZ_PAD2 + 7) / 8 + 16);          // (slot_encode's geometry of two / spc)
    if ((rc = s.mtwo.ensure((size_t)nmask * 2 + 96))) return rc;
    if ((rc = s.mspc.ensure((size_t)nmask + 96))) return rc;
    LZ_HIP(hipMemsetAsync(s.mtwo.p, 0, (size_t)nmask * 2 + 96, c.stream));
    LZ_HIP(hipMemsetAsync(s.mspc.p, 0xFF, (size_t)nmask + 96, c.stream));
    if ((rc = lzk_pack2(c, code_base, s.raw_base(), s.len, s.mtwo.as<u8>(), s.mspc.as<u8>(), nmask, reinterpret_cast<u32*>(tmp + 256)))) return rc;
    s.match_key = key;
    return 0;
}

// (the two helpers of B3's set-up: on B3's stream, with B3's own class-table buffer and timer)
int lz_slot_upload_public(LzCtx& c, SeqSlot& s, const u8* bytes, u32 len) { return slot_upload(c, s, bytes, len, false, c.dp_stream); }
int lz_encode_with(LzCtx& c, const u8* raw, u8* code, u32 len, const u8 cls[256])
{
    int rc = c.cls_tmp.ensure(256); if (rc) return rc;
    LZ_HIP(hipMemcpyAsync(c.cls_tmp.p, cls, 256, hipMemcpyHostToDevice, c.dp_stream));
    LZ_HIP(hipStreamSynchronize(c.dp_stream));
    if ((rc = lzk_encode(c, raw, code, len, c.cls_tmp.as<u8>(), c.dp_stream, &c.dp_timer))) return rc;
    LZ_HIP(hipStreamSynchronize(c.dp_stream));
    return 0;
}
SeqSlot* lz_query_slot(LzCtx& c, int slot, bool create)
{
    std::lock_guard<std::mutex> lk(c.slots_m);
    if (create) return &c.queries[slot];
    auto it = c.queries.find(slot);
    return it == c.queries.end() ? nullptr : &it->second;
}

extern "C" int lzgpu_query_upload(int32_t slot, const uint8_t* q, uint32_t qlen)
{
    int rc = require_init(); if (rc) return rc;
    if (slot < 0 || !q) return lz_fail(LZGPU_ERR_ARG, "bad query slot");
    if (qlen >= 0x7FFFFFFFu) return LZGPU_NH_SIZE;
    return slot_upload(g_ctx, *lz_query_slot(g_ctx, slot, true), q, qlen, true);
}

// ------------------------------------------------------------------------------ B1

extern "C" int lzgpu_table_prepare(const uint8_t* t, uint32_t tlen, uint32_t start, uint32_t end,
                                   const int8_t char_to_bits[256], const lz_seed_desc* seed, uint32_t step)
{
    int rc = require_init(); if (rc) return rc;
    LzCtx& c = g_ctx;
    if (!t || !seed || !char_to_bits) return lz_fail(LZGPU_ERR_ARG, "null argument");
    if (step < 1) return lz_fail(LZGPU_ERR_ARG, "in build_seed_position_table(), step can't be %u", step);
    if (end == 0) end = tlen;
    if (end <= start) return lz_fail(LZGPU_ERR_ARG, "interval is void (%u..%u)", start, end);
    if (end > tlen)   return lz_fail(LZGPU_ERR_ARG, "interval end is bad (%u>%u)", end, tlen);
    if (tlen >= 0x7FFFFFFFu) return LZGPU_NH_SIZE;
    if ((rc = lzh_seed_to_dev(seed, c.seed))) return rc;

    c.have_table = false;
    lz_limit_lift(c);
    memset(&c.geom, 0, sizeof(c.geom));
    c.geom.tlen = tlen; c.geom.start = start; c.geom.end = end; c.geom.step = step; c.geom.seed = *seed;
    memcpy(c.geom.char_to_bits, char_to_bits, 256);
    if ((rc = slot_upload(c, c.target, t, tlen, true))) return rc;
    u8 cls[256]; lzh_make_cls(nullptr, char_to_bits, cls);
    if ((rc = slot_encode(c, c.target, cls, c.cls_t))) return rc;
    if ((rc = lzk_table_build(c))) return rc;
    c.geom.num_words = c.num_words;
    c.have_table = true;
    return 0;
}

extern "C" int lzgpu_target_upload(const uint8_t* t, uint32_t tlen)
{
    int rc = require_init(); if (rc) return rc;
    LzCtx& c = g_ctx;
    if (!t) return lz_fail(LZGPU_ERR_ARG, "null argument");
    if (tlen >= 0x7FFFFFFFu) return LZGPU_NH_SIZE;
    c.have_table = false;
    lz_limit_lift(c);
    memset(&c.geom, 0, sizeof(c.geom));
    c.geom.tlen = tlen;
    return slot_upload(c, c.target, t, tlen, true);
}

// A few bytes of the resident target overwritten in place (the fences lastz puts around a chore's target interval,
// src/sequences.c:7789-7828, and their removal).  The position table is left as it is; every encoding of the target is
// made again by the next call that needs it, and so is wctx.
extern "C" int lzgpu_target_patch(const uint32_t* pos, const uint8_t* bytes, uint32_t n)
{
    int rc = require_init(); if (rc) return rc;
    LzCtx& c = g_ctx;
    if (n && (!pos || !bytes)) return lz_fail(LZGPU_ERR_ARG, "null argument");
    if (!c.target.have_raw || c.target.host.size() != c.target.len) return lz_fail(LZGPU_ERR_STATE, "no target on the device");
    for (u32 k = 0; k < n; k++) if (pos[k] >= c.target.len) return lz_fail(LZGPU_ERR_ARG, "target position %u is past the end (%u)", pos[k], c.target.len);
    if (!n) return 0;
    for (u32 k = 0; k < n; k++) {
        c.target.host[pos[k]] = bytes[k];
        LZ_HIP(hipMemcpyAsync(c.target.raw_base() + pos[k], &c.target.host[pos[k]], 1, hipMemcpyHostToDevice, c.stream));
    }
    LZ_HIP(hipStreamSynchronize(c.stream));
    c.target.code_key = 0; c.target.dp_key = 0; c.target.match_key = 0;
    c.wctx_gen = 0; c.wctx_code_key = 0;
    return 0;
}

// The range form of lzgpu_target_patch: len bytes from `start` on, in one copy (the bases dynamic masking turns into 'x').
extern "C" int lzgpu_target_update(uint32_t start, const uint8_t* bytes, uint32_t len)
{
    int rc = require_init(); if (rc) return rc;
    LzCtx& c = g_ctx;
    if (len && !bytes) return lz_fail(LZGPU_ERR_ARG, "null argument");
    if (!c.target.have_raw || c.target.host.size() != c.target.len) return lz_fail(LZGPU_ERR_STATE, "no target on the device");
    if (start > c.target.len || len > c.target.len - start) return lz_fail(LZGPU_ERR_ARG, "target range %u+%u is past the end (%u)", start, len, c.target.len);
    if (!len) return 0;
    memcpy(&c.target.host[start], bytes, len);
    LZ_HIP(hipMemcpyAsync(c.target.raw_base() + start, &c.target.host[start], len, hipMemcpyHostToDevice, c.stream));
    LZ_HIP(hipStreamSynchronize(c.stream));
    c.target.code_key = 0; c.target.dp_key = 0; c.target.match_key = 0;
    c.wctx_gen = 0; c.wctx_code_key = 0;
    return 0;
}

// ---- dynamic masking (lastz --masking=<count>)
// mask_seed_position_table (src/pos_table.c:747-887; called through mask_interval's callback, src/lastz.c:3787-3806) for n
// intervals at once, on the resident table in place (mask_kernels.hip).
extern "C" int lzgpu_table_mask(const lz_interval* iv, uint32_t n)
{
    LzCtx& c = g_ctx;
    if (!c.have_table) return lz_fail(LZGPU_ERR_STATE, "no position table");
    if (n && !iv) return lz_fail(LZGPU_ERR_ARG, "null argument");
    for (u32 k = 0; k < n; k++) {
        if (iv[k].end <= iv[k].start) return lz_fail(LZGPU_ERR_ARG, "interval is void (%u..%u)", iv[k].start, iv[k].end);
        if (iv[k].end > c.geom.tlen)  return lz_fail(LZGPU_ERR_ARG, "interval end is bad (%u>%u)", iv[k].end, c.geom.tlen);
    }
    if (c.limit != 0 || c.n_owners > 1) return LZGPU_NH_UNSUPPORTED;
    if (!n) return 0;
    int rc = lz_bind_thread(); if (rc) return rc;
    return lzk_table_mask(c, iv, n, c.geom.tlen);
}

extern "C" int lzgpu_table_rebuild(void)
{
    LzCtx& c = g_ctx;
    if (!c.have_table) return lz_fail(LZGPU_ERR_STATE, "no position table");
    int rc = lz_bind_thread(); if (rc) return rc;
    lz_limit_lift(c);
    rc = lzk_table_build(c);
    if (!rc) c.geom.num_words = c.num_words;
    return rc;
}

extern "C" uint64_t lzgpu_table_num_words(void) { return g_ctx.have_table ? g_ctx.num_words : 0; }

extern "C" int lzgpu_table_export(uint32_t* last, uint32_t* prev)
{
    LzCtx& c = g_ctx;
    if (!c.have_table) return lz_fail(LZGPU_ERR_STATE, "no position table");
    u32 nwords = 1u << c.seed.weight;
    u32 adj = c.geom.start - (c.geom.start % c.geom.step);
    u32 prev_entries = 1 + (c.geom.end - adj) / c.geom.step;       // src/pos_table.c:1065
    DevBuf dl, dp; int rc;
    if ((rc = lz_bind_thread())) return rc;
    if (last && (rc = dl.ensure((size_t)nwords * 4))) return rc;
    if (prev && (rc = dp.ensure((size_t)prev_entries * 4))) { dl.release(); return rc; }
    rc = lzk_table_export(c, last ? dl.as<u32>() : nullptr, prev ? dp.as<u32>() : nullptr, prev_entries);
    if (!rc) {
        if (last) (void)hipMemcpyAsync(last, dl.p, (size_t)nwords * 4, hipMemcpyDeviceToHost, c.stream);
        if (prev) (void)hipMemcpyAsync(prev, dp.p, (size_t)prev_entries * 4, hipMemcpyDeviceToHost, c.stream);
        if (hipStreamSynchronize(c.stream) != hipSuccess) rc = lz_fail(LZGPU_ERR_HIP, "table export copy failed");
    }
    dl.release(); dp.release();
    return rc;
}

extern "C" int lzgpu_table_geom(lz_table_geom* out)
{
    if (!g_ctx.have_table || !out) return lz_fail(LZGPU_ERR_STATE, "no position table");
    *out = g_ctx.geom; return 0;
}

extern "C" int lzgpu_table_adopt(const lz_table_geom* g)
{
    int rc = require_init(); if (rc) return rc;
    LzCtx& c = g_ctx;
    if (!g) return LZGPU_ERR_ARG;
    lz_limit_lift(c);                                           // (before the seed changes: the buffers go back where they belong)
    if ((rc = lzh_seed_to_dev(&g->seed, c.seed))) return rc;
    c.have_table = false; c.geom = *g; c.num_words = g->num_words; c.table_gen++;
    size_t total = (size_t)g->tlen + 2 * LZ_SEQ_PAD + 16;
    if ((rc = c.target.raw.ensure(total))) return rc;
    if ((rc = c.target.code.ensure(total))) return rc;
    LZ_HIP(hipMemsetAsync(c.target.raw.p, 0, total, c.stream));
    LZ_HIP(hipMemsetAsync(c.target.code.p, LZ_CODE_INVALID, total, c.stream));
    c.target.len = g->tlen; c.target.have_raw = true; c.target.code_key = 0; c.target.dp_key = 0; c.target.match_key = 0; c.target.host.clear();
    if ((rc = c.wstart.ensure(((size_t)(1u << c.seed.weight) + 1) * 4))) return rc;
    if ((rc = c.wpos.ensure((size_t)(g->num_words ? g->num_words : 1) * 4))) return rc;
    LZ_HIP(hipStreamSynchronize(c.stream));
    return 0;
}

extern "C" int lzgpu_table_buffers(void* dev_ptr[3], uint64_t bytes[3])
{
    LzCtx& c = g_ctx;
    if (!c.target.have_raw || !c.wstart.p) return lz_fail(LZGPU_ERR_STATE, "no table buffers");
    dev_ptr[0] = c.target.raw_base(); bytes[0] = c.geom.tlen;
    dev_ptr[1] = c.built_wstart().p;  bytes[1] = ((uint64_t)(1u << c.seed.weight) + 1) * 4;      // (the table as it was built, also under a limit)
    dev_ptr[2] = c.built_wpos().p;    bytes[2] = (uint64_t)c.built_num_words() * 4;
    return 0;
}

extern "C" int lzgpu_table_commit(void)
{
    LzCtx& c = g_ctx;
    if (!c.target.have_raw || !c.wstart.p) return lz_fail(LZGPU_ERR_STATE, "no table buffers");
    { int rc = lz_bind_thread(); if (rc) return rc; }
    lz_limit_lift(c);
    // the entropy finish needs the target bytes on the host as well (the target itself does not
    // change between commits of the same geometry: copied back once)
    if (c.target.host.size() != c.geom.tlen) {
        c.target.host.resize(c.geom.tlen);
        if (c.geom.tlen) LZ_HIP(hipMemcpy(c.target.host.data(), c.target.raw_base(), c.geom.tlen, hipMemcpyDeviceToHost));
        c.target.code_key = 0; c.target.dp_key = 0; c.target.match_key = 0;
    }
    c.table_gen++;                                              // (the caller wrote wpos)
    c.have_table = true;
    return 0;
}

// ---- the word-count limit (lastz --maxwordcount)
// limit_position_table(pt, limit, 0) (src/pos_table.c:1763-1948; called at src/lastz.c:1219-1221): the searches read a copy of
// the table without the lists of more than `limit` entries; the table as it was built stays where export / geom / buffers /
// save / share find it, and every call that makes a table ends the limit.
extern "C" int lzgpu_table_limit(uint32_t limit)
{
    LzCtx& c = g_ctx;
    if (!c.have_table) return lz_fail(LZGPU_ERR_STATE, "no position table");
    int rc = lz_bind_thread(); if (rc) return rc;
    if (limit == c.limit) return 0;
    lz_limit_lift(c);
    return limit ? lzk_table_limit(c, limit) : 0;
}

// position_table_count_distribution (src/pos_table.c:2064-2140) of the table as it was built.  Both out arrays are released
// with lzgpu_free().
extern "C" int lzgpu_table_count_distribution(uint32_t** count, uint32_t** words, uint32_t* n)
{
    LzCtx& c = g_ctx;
    if (!count || !words || !n) return lz_fail(LZGPU_ERR_ARG, "null argument");
    *count = *words = nullptr; *n = 0;
    if (!c.have_table) return lz_fail(LZGPU_ERR_STATE, "no position table");
    int rc = lz_bind_thread(); if (rc) return rc;
    std::vector<u32> cn, wd;
    if ((rc = lzk_table_count_distribution(c, cn, wd))) return rc;
    const size_t bytes = (cn.size() ? cn.size() : 1) * sizeof(u32);
    u32* a = (u32*)malloc(bytes); u32* b = (u32*)malloc(bytes);
    if (!a || !b) { free(a); free(b); return lz_fail(LZGPU_ERR_OOM, "host malloc failed"); }
    if (!cn.empty()) { memcpy(a, cn.data(), cn.size() * sizeof(u32)); memcpy(b, wd.data(), wd.size() * sizeof(u32)); }
    *count = a; *words = b; *n = (uint32_t)cn.size();
    return 0;
}

// find_position_table_limit(pt, keep) (src/pos_table.c:2000-2034; called at src/lastz.c:1215-1218) on the table as it was
// built, in the reference's own arithmetic: unspos (u32) products and sums, the float product numPositions * keep, ceil in double
extern "C" int lzgpu_table_find_limit(float keep, uint32_t* limit)
{
    LzCtx& c = g_ctx;
    if (!limit) return lz_fail(LZGPU_ERR_ARG, "null argument");
    *limit = 0;
    if (!c.have_table) return lz_fail(LZGPU_ERR_STATE, "no position table");
    int rc = lz_bind_thread(); if (rc) return rc;
    std::vector<u32> cn, wd;
    if ((rc = lzk_table_count_distribution(c, cn, wd))) return rc;
    u32 num_positions = 0;
    for (size_t k = 0; k < cn.size(); k++) num_positions += cn[k] * wd[k];
    const float prod = (float)num_positions * keep;             // (numPositions * keep: unspos times float is a float product)
    u32 min_to_keep = (u32)ceil((double)prod);
    for (size_t k = 0; k < cn.size(); k++) {
        if (cn[k] * wd[k] >= min_to_keep) { *limit = cn[k]; break; }
        min_to_keep -= cn[k] * wd[k];
    }
    return 0;
}

extern "C" int lzgpu_device_copy(void* dst, const void* src, uint64_t bytes)
{
    int rc = require_init(); if (rc) return rc;
    if (!bytes) return 0;
    LZ_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, g_ctx.stream));
    LZ_HIP(hipStreamSynchronize(g_ctx.stream));
    return 0;
}

// ------------------------------------------------------------------------------ B2

#include <chrono>
struct HostProf {
    bool on = false; double t[16]; const char* names[16] = { nullptr }; int n = 0;
    std::chrono::steady_clock::time_point last;
    HostProf() { for (auto& x : t) x = 0; }
    void start() { on = lz_settings().hostprof; if (on) last = std::chrono::steady_clock::now(); }
    void lap(int k, const char* name) {
        if (!on) return;
        auto now = std::chrono::steady_clock::now();
        t[k] += std::chrono::duration<double, std::milli>(now - last).count(); names[k] = name; if (k >= n) n = k + 1; last = now;
    }
    ~HostProf() { if (on) for (int k = 0; k < n; k++) if (names[k]) fprintf(stderr, "[lzgpu hostprof] %-28s %10.2f ms total\n", names[k], t[k]); }
};
static HostProf g_hp;

// wctx (lz_ctx.hpp) for the table and the target codes as they are now: rebuilt when either changed since it was
// built.  It is not to crowd out the per-chunk buffers: when it would take more than half of the device memory that
// is free (counting what it holds already), or the allocation fails, `fused` comes back false and the search runs
// the two kernels -- no error.
static int lz_wctx_prepare(LzCtx& c, bool& fused)
{
    if (c.wctx.p && c.wctx_gen == c.table_gen && c.wctx_code_key == c.target.code_key && c.target.code_key) return 0;
    const size_t need = (size_t)c.num_words * LZ_WCTX_BYTES;
    if (c.num_words == 0) { fused = false; return 0; }
    if (need > c.wctx.cap || !c.wctx.p) {
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) != hipSuccess || need > (fr + c.wctx.cap) / 2 || c.wctx.ensure(need) != 0) {
            (void)hipGetLastError(); c.last_error.clear();
            c.wctx_gen = 0; c.wctx_code_key = 0;
            fused = false;
            return 0;
        }
    }
    c.wctx_gen = 0; c.wctx_code_key = 0;
    int rc = lzk_wctx_build(c);
    if (rc) return rc;
    c.wctx_gen = c.table_gen; c.wctx_code_key = c.target.code_key;
    return 0;
}

// The query of a search: the caller's bytes, uploaded into the transient slot -1 (not when `upload` is false: the self
// entry point asks for the length ahead of seed_search, qs stays null), or a resident slot.
static int lz_search_query(LzCtx& c, const u8* bytes, u32 len, int slot, bool upload, SeqSlot*& qs, u32& qlen)
{
    qs = nullptr; qlen = len;
    if (bytes) {
        if (!upload) return 0;
        if (len >= 0x7FFFFFFFu) return LZGPU_NH_SIZE;
        qs = lz_query_slot(c, -1, true);
        return slot_upload(c, *qs, bytes, len, false);
    }
    qs = slot < 0 ? nullptr : lz_query_slot(c, slot, false);
    if (!qs) return lz_fail(LZGPU_ERR_ARG, "query slot %d is empty", slot);
    qlen = qs->len;
    return 0;
}

// a result list as the ABI hands it out (lzgpu_free)
static int lz_hsps_out(const std::vector<lz_hsp>& v, lz_hsp** out, uint64_t* n_out)
{
    lz_hsp* res = (lz_hsp*)malloc((v.size() ? v.size() : 1) * sizeof(lz_hsp));
    if (!res) return lz_fail(LZGPU_ERR_OOM, "host malloc failed");
    if (!v.empty()) memcpy(res, v.data(), v.size() * sizeof(lz_hsp));
    *out = res; *n_out = v.size();
    return 0;
}

// what both seed-search entry points begin with (args_ok: the caller's test of its pointers)
static int search_enter(bool args_ok, lz_hsp** out, uint64_t* n_out)
{
    int rc = require_init(); if (rc) return rc;
    if (!args_ok) return lz_fail(LZGPU_ERR_ARG, "null argument");
    *out = nullptr; *n_out = 0; g_ctx.filter_dropped = 0;
    if (!g_ctx.have_table) return lz_fail(LZGPU_ERR_STATE, "lzgpu_table_prepare has not been called");
    return 0;
}

struct SeedSearch {                                             // a seed_search in progress: what its steps hand on
    const lz_search_args* a;
    SeqSlot* qs = nullptr; const u8* qhost = nullptr;           // the query on the device and on the host
    u32 lo = 0, hi = 0, n = 0, L = 0;                           // the interval of query positions, its length, the seed's length
    u64 total_hits = 0;
    std::vector<LzChunk> chunks; u64 max_chunk = 0;             // [i0,i1) in query positions with at most hit_capacity hits each
    int mode = 2; bool fused = false;                           // phase-A scan mode; k_scan_hits2 in the place of fill + scan
    const int8_t* match_bits = nullptr;                         // an exact-match search (lzgpu_seed_hit_search_exact): a->sub, xdrop, entropic and extend are not read
    u32 mismatches = 0;                                         // ... or, not 0, an N-mismatch search (lzgpu_seed_hit_search_mismatch), on the same match codes
    bool exact() const { return match_bits != nullptr; }
    bool extend() const { return exact() || a->extend != 0; }
    LzExtendParams P; LzLutParams Q; LzExactParams X; LzMismatchParams MM;
    bool filtered = false; LzFilterParams F;                    // a hit filter is in force (lzgpu_set_hit_filter): every chunk's keys pass lzk_filter_hits
    u32 out_cap = 0;
    std::vector<lz_hsp> plain;                                  // !a->extend: every hit
};

// ---- 1. the query and the interval of it to search
static int ss_query(LzCtx& c, SeedSearch& s)
{
    const lz_search_args* a = s.a;
    u32 qlen;
    int rc = lz_search_query(c, a->query, a->qlen, a->query_slot, true, s.qs, qlen); if (rc) return rc;
    s.qhost = a->query ? a->query : s.qs->host.data();
    s.lo = a->start; s.hi = a->end ? a->end : qlen;
    if (s.hi <= s.lo) return lz_fail(LZGPU_ERR_ARG, "in seed_hit_search(), interval is void (%u-%u)", s.lo, s.hi);
    if (s.hi > qlen) return lz_fail(LZGPU_ERR_ARG, "in seed_hit_search(), interval end is bad (%u>%u)", s.hi, qlen);
    s.n = s.hi - s.lo; s.L = (u32)c.seed.length;
    g_hp.lap(7, "query slot");
    return 0;
}

// ---- 2. scoring classes and the codes of both sequences
// (the class compression and the 4 KiB table upload are skipped when the caller passes the same
// matrix as last time -- lastz passes maskedScoring for every strand of every query)
static int ss_classes(LzCtx& c, SeedSearch& s)
{
    const s32* sub = s.a->sub;
    int rc;
    if (s.exact()) {
        // the codes the enumeration reads (the table's char_to_bits, no score classes) and the match codes of both sequences
        u8 cls[256];
        lzh_make_cls(nullptr, c.geom.char_to_bits, cls);
        if ((rc = slot_encode(c, c.target, cls, c.cls_t))) return rc;
        if ((rc = slot_encode(c, *s.qs, cls, c.cls_q))) return rc;
        if ((rc = slot_match_encode(c, c.target, s.match_bits))) return rc;
        if ((rc = slot_match_encode(c, *s.qs, s.match_bits))) return rc;
        g_hp.lap(0, "upload+classes+encode");
        return 0;
    }
    if (c.score_sub.size() != 65536 || memcmp(c.score_sub.data(), sub, 65536 * sizeof(s32)) != 0) {
        s32 tab[LZ_NCLASS * LZ_NCLASS];
        c.score_sub.clear();
        if ((rc = lzh_score_classes(sub, c.rowc, c.colc, tab))) return rc;
        if ((rc = c.score_tab.ensure(sizeof(tab)))) return rc;
        LZ_HIP(hipMemcpyAsync(c.score_tab.p, tab, sizeof(tab), hipMemcpyHostToDevice, c.stream));
        LZ_HIP(hipStreamSynchronize(c.stream));
        c.score_sub.assign(sub, sub + 65536);
    }
    g_hp.lap(8, "score classes + table upload");
    u8 cls[256];
    lzh_make_cls(c.rowc, c.geom.char_to_bits, cls);
    if ((rc = slot_encode(c, c.target, cls, c.cls_t))) return rc;
    lzh_make_cls(c.colc, c.geom.char_to_bits, cls);
    if ((rc = slot_encode(c, *s.qs, cls, c.cls_q))) return rc;
    if (s.filtered) {                                           // the match codes the filter reads, beside the scoring codes (one encode pass each, cached by match_bits)
        if ((rc = slot_match_encode(c, c.target, c.filter.match_bits))) return rc;
        if ((rc = slot_match_encode(c, *s.qs, c.filter.match_bits))) return rc;
    }
    g_hp.lap(0, "upload+classes+encode");
    return 0;
}

// ---- 3. per query position: the raw hits and their exclusive scan; the total and sampled prefix sums on the host
static const u32 LZ_PLAN_STRIDE = 4096;
static int ss_count(LzCtx& c, SeedSearch& s)
{
    const u32 n = s.n;
    int rc;
    if ((rc = c.cnt.ensure((size_t)n * 4))) return rc;
    if ((rc = c.off.ensure((size_t)n * 8))) return rc;
    if ((rc = c.pk.ensure((size_t)n * 4))) return rc;
    if ((rc = c.wiv.ensure((size_t)n * 4))) return rc;
    if ((rc = c.wsk.ensure((size_t)n * 4))) return rc;
    if ((rc = c.wsv.ensure((size_t)n * 4))) return rc;
    if ((rc = c.diag_end.ensure((size_t)LZ_DIAG_SIZE * 4))) return rc;
    if ((rc = c.dev_counters.ensure(8 * 8))) return rc;
    if ((rc = c.hsp_count.ensure(4))) return rc;
    LZ_HIP(hipMemsetAsync(c.diag_end.p, 0, (size_t)LZ_DIAG_SIZE * 4, c.stream));      // empty_diag_hash
    LZ_HIP(hipMemsetAsync(c.dev_counters.p, 0, 64, c.stream));                        // [0]=extensions [1]=bp [2]=words
    LZ_HIP(hipMemsetAsync(c.hsp_count.p, 0, 4, c.stream));

    if ((rc = lzk_count_hits(c, s.qs->code_base(), s.lo, s.hi))) return rc;
    if ((rc = lzk_scan_counts(c, n))) return rc;

    // total and the sampled prefix sums for the chunk plan come back through pinned memory the device
    // writes itself: one synchronisation, no staged device-to-host copies
    const u32 ns = (n + LZ_PLAN_STRIDE - 1) / LZ_PLAN_STRIDE;
    if (c.pinned_words < (size_t)ns + 16) {
        if (c.pinned) (void)hipHostFree(c.pinned);
        c.pinned = nullptr; c.pinned_words = 0;
        LZ_HIP(hipHostMalloc((void**)&c.pinned, ((size_t)ns + 16) * 8, hipHostMallocDefault));
        c.pinned_words = (size_t)ns + 16;
    }
    if ((rc = lzk_sample_offsets(c, n, LZ_PLAN_STRIDE, ns))) return rc;
    c.blk_start_host.assign((size_t)c.blk_count + 1, 0);       // (a chunk's launch of the fill kernel covers its blocks' range of the sorted list)
    LZ_HIP(hipMemcpyAsync(c.blk_start_host.data(), c.blk_start.p, ((size_t)c.blk_count + 1) * 8, hipMemcpyDeviceToHost, c.stream));
    LZ_HIP(hipStreamSynchronize(c.stream));
    g_hp.lap(1, "count+scan (sync)");
    c.timer.resolve();
    s.total_hits = c.pinned[0];
    return 0;
}

// ---- 4. chunk plan.  Prefix sums are sampled every LZ_PLAN_STRIDE positions; finer values are fetched only if a
// single block of that many positions exceeds the capacity.
static int ss_plan(LzCtx& c, SeedSearch& s)
{
    const u64* samp = c.pinned + 1;
    hipError_t fetch_err = hipSuccess;
    auto off_at = [&](u32 i) -> u64 {
        if (i >= s.n) return s.total_hits;
        if (i % LZ_PLAN_STRIDE == 0) return samp[i / LZ_PLAN_STRIDE];
        u64 v = 0;
        hipError_t e = hipMemcpy(&v, c.off.as<u64>() + i, 8, hipMemcpyDeviceToHost);
        if (e != hipSuccess) fetch_err = e;
        return v;
    };
    int rc = lzh_plan_chunks(s.n, c.hit_capacity, LZ_PLAN_STRIDE, off_at, s.chunks); if (rc) return rc;
    if (fetch_err != hipSuccess) return lz_fail(LZGPU_ERR_HIP, "prefix fetch failed: %s", hipGetErrorString(fetch_err));
    for (auto& ch : s.chunks) if (ch.nh > s.max_chunk) s.max_chunk = ch.nh;
    g_hp.lap(2, "chunk plan");
    return 0;
}

// ---- 5. the kernels' parameters, the scan mode and its look-up tables.
// Phase A: four bases per step on 2-bit codes when the matrix, xDrop and the bytes that occur allow it
// (mode 0 / 1 = without / with special-byte masks), else the byte-code scans (mode 2)
static int ss_scan_mode(LzCtx& c, SeedSearch& s)
{
    const lz_search_args* a = s.a;
    SeqSlot* qs = s.qs;
    if (s.filtered) {
        LzFilterParams& F = s.F;
        F.t2 = c.target.mtwo.as<u8>(); F.tsp = c.target.mspc.as<u8>(); F.q2 = qs->mtwo.as<u8>(); F.qsp = qs->mspc.as<u8>();
        F.pos_spread = lz_filter_spread(c.filter.positions); F.seed_len = s.L;
        F.min_matches = c.filter.min_matches; F.max_transversions = c.filter.max_transversions;
    }
    if (s.exact()) {                                            // k_scan_exact: no mode, no tables, never fused
        LzExactParams& X = s.X;
        X.t2 = c.target.mtwo.as<u8>(); X.tsp = c.target.mspc.as<u8>(); X.q2 = qs->mtwo.as<u8>(); X.qsp = qs->mspc.as<u8>();
        X.tlen = c.geom.tlen; X.qlen = qs->len; X.seed_len = s.L; X.thr = (u32)a->hsp_threshold;      // src/seed_search.c:3209
        s.MM.X = X; s.MM.traw = c.target.raw_base(); s.MM.qraw = qs->raw_base(); s.MM.M = s.mismatches;      // (the bytes k_hsp_match_counts reads, too)
        s.fused = false;
        return 0;
    }
    LzExtendParams& P = s.P; LzLutParams& Q = s.Q;
    P.tcode = c.target.code_base(); P.tlen = c.geom.tlen;
    P.qcode = qs->code_base();      P.qlen = qs->len;
    P.xdrop = a->xdrop; P.min_score = a->hsp_threshold; P.seed_len = s.L;
    P.cls8 = lzh_small_classes(c.rowc, c.colc);
    const bool nibs = P.cls8 && c.target.have_nib && qs->have_nib;
    P.tnib = nibs ? c.target.nib.as<u8>() : nullptr; P.qnib = nibs ? qs->nib.as<u8>() : nullptr;
    Q.t2 = c.target.two.as<u8>(); Q.q2 = qs->two.as<u8>(); Q.tsp = c.target.spc.as<u8>(); Q.qsp = qs->spc.as<u8>(); Q.xdrop = a->xdrop;
    Q.t2x = c.target.two_x.as<u8>(); Q.tspx = c.target.spc_x.as<u8>();
    Q.tcode = P.tcode; Q.qcode = P.qcode;

    int mode = 2, rc;
    if (a->extend) {
        s32 M4[16];
        if (lzh_lut_eligible(a->sub, c.geom.char_to_bits, c.target.occ, qs->occ, a->xdrop, M4))
            mode = (c.target.has_special || qs->has_special) ? 1 : 0;
        if (mode < c.min_scan_mode) mode = c.min_scan_mode;         // lzgpu_set_scan_mode (tests): 1 = masks even without specials, 2 = byte-code scans
        if (mode < 2 && (c.lut_xdrop != a->xdrop || c.lut_m4.size() != 16 || memcmp(c.lut_m4.data(), M4, sizeof(M4)) != 0)) {
            std::vector<LzLutEntry> lut_host(LZ_LUT_TOTAL);
            c.lut_m4.clear();
            lzh_lut_build(M4, a->xdrop, lut_host.data());
            if ((rc = c.lut.ensure(lut_host.size() * sizeof(LzLutEntry)))) return rc;
            LZ_HIP(hipMemcpyAsync(c.lut.p, lut_host.data(), lut_host.size() * sizeof(LzLutEntry), hipMemcpyHostToDevice, c.stream));
            LZ_HIP(hipStreamSynchronize(c.stream));
            c.lut_m4.assign(M4, M4 + 16); c.lut_xdrop = a->xdrop;
        }
    }
    s.mode = c.last_scan_mode = mode;
    // scan mode 0 takes the fused path (k_scan_hits2: enumeration + phase A over the context-inlined table, tagged
    // records in keys and neither summaries nor partition bytes) unless LZGPU_FUSED_SCAN=0 asks for the two kernels,
    // the fill variant in use is one the fused kernel does not reproduce (bucket owners), a hit filter needs the key stream
    // between the two kernels (lzk_filter_hits), or wctx cannot be had (lz_wctx_prepare)
    s.fused = a->extend && mode == 0 && s.max_chunk && lz_settings().fused_scan && c.n_owners <= 1 && !s.filtered;
    if (s.fused && (rc = lz_wctx_prepare(c, s.fused))) return rc;
    return 0;
}

// ---- 6. the per-chunk buffers, sized once per search for the largest chunk
static int ss_reserve(LzCtx& c, SeedSearch& s)
{
    const bool extend = s.extend();
    const u64 max_chunk = s.max_chunk;
    int rc;
    if (max_chunk) {
        if ((rc = c.keys.ensure((size_t)max_chunk * 8))) return rc;
        if (!s.fused && (rc = c.bins.ensure((size_t)max_chunk + 64))) return rc;       // k_fill_hits writes a partition byte per hit on every path (the plain-hit path included)
        if (s.filtered && (rc = lzk_filter_reserve(c, max_chunk))) return rc;          // (only while a filter is in force: 8 bytes per hit more)
    }
    if (extend && max_chunk) {
        const size_t ntiles = (size_t)((max_chunk + LZ_PP_TILE_HOST - 1) / LZ_PP_TILE_HOST), nblocks = (ntiles + 255) / 256;
        if ((rc = c.bin_base.ensure(257 * 4))) return rc;
        if ((rc = c.hist.ensure(ntiles * 256 * 4))) return rc;
        if ((rc = c.hist_part.ensure(nblocks * 256 * 4))) return rc;
        if ((rc = c.run_addr.ensure(ntiles * 256 * 4))) return rc;
    }
    s.out_cap = (u32)std::min<u64>(c.hsp_capacity, 0xFFFFFFF0ull);
    if (extend && (rc = c.hsp_out.ensure((size_t)s.out_cap * sizeof(LzHspRec)))) return rc;
    if (s.exact()) return max_chunk ? c.summ.ensure((size_t)max_chunk * 4) : 0;
    if (extend && max_chunk && (rc = s.fused ? lzk_fused_reserve(c, max_chunk) : lzk_scan_reserve(c, s.mode, max_chunk))) return rc;
    return 0;
}

// ---- 7. one chunk: enumeration + phase A (one launch or two), the records sorted tile by tile where they lie, the runs'
// ranks from the counts that leaves, phase B.  All on c.stream: diagEnd carries from chunk to chunk, in chunk order.
// (under a hit filter, after the fill: the chunk's keys compacted to those the filter keeps, nh their number from here on)
static int ss_filter(LzCtx& c, SeedSearch& s, u64& nh)
{
    if (!s.filtered) return 0;
    u64 kept = 0;
    int rc = lzk_filter_hits(c, s.F, nh, &kept); if (rc) return rc;
    c.filter_dropped += nh - kept;
    nh = kept;
    return 0;
}
static int ss_chunk(LzCtx& c, SeedSearch& s, const LzChunk& ch)
{
    int rc; u64 nh = ch.nh;
    if (s.fused) {
        if ((rc = lzk_scan_fused(c, s.lo, ch, s.n, s.P, s.Q))) return rc;
    } else {
        if ((rc = lzk_fill_hits(c, s.lo, ch, s.n))) return rc;
        if ((rc = ss_filter(c, s, nh))) return rc;
        if (nh == 0) return 0;                                  // (a chunk without a survivor launches nothing more; diagEnd carries over untouched)
        if ((rc = lzk_scan_hits(c, s.mode, s.P, s.Q, nh))) return rc;
    }
    if ((rc = lzk_partition(c, s.fused, nh))) return rc;
    if ((rc = lzk_hist_scan(c, nh))) return rc;
    return lzk_settle(c, s.P, nh, s.out_cap);
}
// ... of an exact-match search: k_scan_exact and k_settle_exact in the places of the X-drop kernels, everything between them as it is;
// of an N-mismatch search: k_scan_mismatch and k_settle_mismatch there
static int ss_chunk_exact(LzCtx& c, SeedSearch& s, const LzChunk& ch)
{
    int rc; u64 nh = ch.nh;
    if ((rc = lzk_fill_hits(c, s.lo, ch, s.n))) return rc;
    if ((rc = ss_filter(c, s, nh))) return rc;
    if (nh == 0) return 0;
    if ((rc = s.mismatches ? lzk_scan_mismatch(c, s.MM, nh) : lzk_scan_exact(c, s.X, nh))) return rc;
    if ((rc = lzk_partition(c, false, nh))) return rc;
    if ((rc = lzk_hist_scan(c, nh))) return rc;
    return s.mismatches ? lzk_settle_mismatch(c, s.MM, nh, s.out_cap) : lzk_settle_exact(c, s.X, nh, s.out_cap);
}
// ... of a search without extension (process_for_plain_hit): every hit is reported
static int ss_chunk_plain(LzCtx& c, SeedSearch& s, const LzChunk& ch)
{
    int rc = lzk_fill_hits(c, s.lo, ch, s.n); if (rc) return rc;
    u64 nh = ch.nh;
    if ((rc = ss_filter(c, s, nh))) return rc;
    if (nh == 0) return 0;
    std::vector<u64> hk(nh);
    LZ_HIP(hipMemcpyAsync(hk.data(), c.keys.p, (size_t)nh * 8, hipMemcpyDeviceToHost, c.stream));
    LZ_HIP(hipStreamSynchronize(c.stream));
    for (u64 k : hk) { u32 p2 = (u32)k; s.plain.push_back({ p2 + (u32)(k >> 32), p2, s.L, 0 }); }
    return 0;
}

// ---- 8. counters; the candidates' match counts; host finish: discovery order, entropy, threshold
static int ss_finish(LzCtx& c, SeedSearch& s, lz_hsp** out, uint64_t* n_out)
{
    const lz_search_args* a = s.a;
    int rc;
    u64 hc[3] = { 0, 0, 0 }; u32 n_rec = 0;
    LZ_HIP(hipMemcpyAsync(hc, c.dev_counters.p, 24, hipMemcpyDeviceToHost, c.stream));
    LZ_HIP(hipMemcpyAsync(&n_rec, c.hsp_count.p, 4, hipMemcpyDeviceToHost, c.stream));
    LZ_HIP(hipStreamSynchronize(c.stream));
    g_hp.lap(4, "wait for GPU");
    // (an exact-match search needs the discovery order only: of k_hsp_match_counts' output the probe index; score = length, no
    // entropy, and the threshold was applied where the length was found)
    const bool extend = s.extend();
    const s32 K = s.exact() ? 0 : a->hsp_threshold;
    const int entropic = s.exact() ? 0 : a->entropic;
    const bool gpu_counts = extend && n_rec > 0 && n_rec <= s.out_cap;
    if (gpu_counts) {
        if ((rc = c.hsp_mc.ensure((size_t)n_rec * 20))) return rc;
        if ((rc = lzk_hsp_match_counts(c, n_rec, *s.qs))) return rc;
    }
    c.timer.resolve();
    { std::lock_guard<std::mutex> lk(c.counters_m);
      c.counters.words += hc[2]; c.counters.raw_hits += s.total_hits;
      c.counters.extensions += hc[0]; c.counters.bp_extended += hc[1]; }
    if (!extend) return lz_hsps_out(s.plain, out, n_out);
    if (n_rec > s.out_cap) return LZGPU_NH_HSP_OVERFLOW;

    std::vector<LzHspRec> recs(n_rec);
    std::vector<u32> mc;
    if (n_rec) LZ_HIP(hipMemcpyAsync(recs.data(), c.hsp_out.p, (size_t)n_rec * sizeof(LzHspRec), hipMemcpyDeviceToHost, c.stream));
    if (gpu_counts) { mc.resize((size_t)n_rec * 5); LZ_HIP(hipMemcpyAsync(mc.data(), c.hsp_mc.p, (size_t)n_rec * 20, hipMemcpyDeviceToHost, c.stream)); }
    LZ_HIP(hipStreamSynchronize(c.stream));
    c.timer.resolve();
    g_hp.lap(5, "copy candidates");
    std::vector<lz_hsp> fin;
    if ((rc = lzh_finish_hsps(recs.data(), n_rec, c.target.host.data(), s.qhost, c.seed, c.geom.char_to_bits,
                              K, entropic, fin, gpu_counts ? mc.data() : nullptr, &c.last_order)))
        return lz_fail(rc, "internal: candidate HSP is not on a seed hit");
    if ((rc = lz_hsps_out(fin, out, n_out))) return rc;
    { std::lock_guard<std::mutex> lk(c.counters_m); c.counters.hsps += fin.size(); }
    g_hp.lap(6, "host finish (order+entropy)");
    return 0;
}

// The hit filter in force against the resident seed and this search, before any work (include/lzgpu.h, lzgpu_set_hit_filter)
static int filter_check(LzCtx& c, const int8_t* match_bits)
{
    if (!c.filter_on) return 0;
    const lz_hit_filter& f = c.filter;
    const u32 L = (u32)c.seed.length;
    if (f.positions == 0 || (L < 32 && (f.positions >> L) != 0)) return lz_fail(LZGPU_ERR_ARG, "hit filter: positions %08x of a seed of length %u", f.positions, L);
    if (f.min_matches < 0 || f.min_matches > __builtin_popcount(f.positions))
        return lz_fail(LZGPU_ERR_ARG, "hit filter: %d matches of %d positions", (int)f.min_matches, __builtin_popcount(f.positions));    // src/lastz.c:9797
    if (match_bits && memcmp(match_bits, f.match_bits, 256) != 0)
        return lz_fail(LZGPU_ERR_ARG, "hit filter: the search's match_bits differ from the filter's (a slot holds one set of match codes)");
    if (c.n_owners > 1) return LZGPU_NH_UNSUPPORTED;             // (the owner path is not tested with the filter kernels)
    return 0;
}

// the search proper (after search_enter); with c.self.mode != LZ_SELF_OFF the count, fill and fused scan kernels drop
// the hits a self-comparison drops
static int seed_search(const lz_search_args* a, lz_hsp** out, uint64_t* n_out, const int8_t* match_bits = nullptr, u32 mismatches = 0)
{
    LzCtx& c = g_ctx;
    SeedSearch s; s.a = a; s.match_bits = match_bits; s.mismatches = mismatches;
    int rc;
    c.filter_dropped = 0;
    if ((rc = filter_check(c, match_bits))) return rc;
    s.filtered = c.filter_on;
    g_hp.start();
    if ((rc = ss_query(c, s))) return rc;
    if ((rc = ss_classes(c, s))) return rc;
    if (s.qs->len < s.L) return 0;                              // src/seed_search.c:486-487
    if ((rc = ss_count(c, s))) return rc;
    if ((rc = ss_plan(c, s))) return rc;
    if ((rc = ss_scan_mode(c, s))) return rc;
    if ((rc = ss_reserve(c, s))) return rc;
    for (const LzChunk& ch : s.chunks) if ((rc = s.exact() ? ss_chunk_exact(c, s, ch) : a->extend ? ss_chunk(c, s, ch) : ss_chunk_plain(c, s, ch))) return rc;
    g_hp.lap(3, "chunk loop launches");
    return ss_finish(c, s, out, n_out);
}

extern "C" int lzgpu_seed_hit_search(const lz_search_args* a, lz_hsp** out, uint64_t* n_out)
{
    int rc = search_enter(a && out && n_out && a->sub, out, n_out);
    return rc ? rc : seed_search(a, out, n_out);
}

// Exact-match extension (lastz --exact=<length>: process_for_simple_hit with gfExtend == gfexExact, src/seed_search.c:1056-1192,
// match_extend_seed_hit, :3018-3254).  Enumeration, the bucket streams, the tile sort and the run tables are the plain search's;
// phase A and phase B are k_scan_exact and k_settle_exact on the match codes of both sequences (lz_exact.hpp).
extern "C" int lzgpu_seed_hit_search_exact(const lz_search_args* a, const int8_t match_bits[256], lz_hsp** out, uint64_t* n_out)
{
    int rc = search_enter(a && match_bits && out && n_out, out, n_out); if (rc) return rc;
    if (g_ctx.n_owners > 1) return LZGPU_NH_UNSUPPORTED;         // (the owner path is not tested with these kernels)
    return seed_search(a, out, n_out, match_bits);
}

// N-mismatch extension (lastz --mismatch=<count>,<length>: process_for_simple_hit with gfExtend in gfexMismatch_min..gfexMismatch_max,
// src/seed_search.c:1056-1192, mismatch_extend_seed_hit, :3450-3778).  As the exact-match search, on the same match codes, with
// k_scan_mismatch and k_settle_mismatch (lz_mismatch.hpp); a->hsp_threshold is the length (:3703).
extern "C" int lzgpu_seed_hit_search_mismatch(const lz_search_args* a, const int8_t match_bits[256], int32_t max_mismatches, lz_hsp** out, uint64_t* n_out)
{
    int rc = search_enter(a && match_bits && out && n_out, out, n_out); if (rc) return rc;
    if (max_mismatches < 1 || max_mismatches > (int32_t)LZ_MM_MAX) return lz_fail(LZGPU_ERR_ARG, "in seed_hit_search_mismatch(), %d mismatches (1..%u)", (int)max_mismatches, LZ_MM_MAX);
    if (a->hsp_threshold < 1) return lz_fail(LZGPU_ERR_ARG, "in seed_hit_search_mismatch(), length %d", (int)a->hsp_threshold);
    if (g_ctx.n_owners > 1) return LZGPU_NH_UNSUPPORTED;         // (as lzgpu_seed_hit_search_exact)
    return seed_search(a, out, n_out, match_bits, (u32)max_mismatches);
}

// Self-comparison (lastz --self, --band).  Every raw hit the reference drops (src/seed_search.c:841-848, 903-908,
// 2052-2235) lies outside an interval of target positions that depends on the query position alone (lz_common.hpp,
// lz_self_bounds), and the table's lists are sorted by position: the count and fill kernels clip each list to that
// interval, and everything after them runs unchanged on the surviving hits.
extern "C" int lzgpu_seed_hit_search_self(const lz_search_args* a, const lz_self_args* s, lz_hsp** out, uint64_t* n_out)
{
    int rc = search_enter(a && s && out && n_out && a->sub, out, n_out); if (rc) return rc;
    LzCtx& c = g_ctx;
    SeqSlot* qs; u32 qlen;                                      // (the length only: seed_search uploads a host-pointer query)
    if ((rc = lz_search_query(c, a->query, a->qlen, a->query_slot, false, qs, qlen))) return rc;
    // what the kernels assume (seed_hit_below_diagonal's note (1), :2068-2070): one sequence against itself
    if (qlen != c.geom.tlen) return LZGPU_NH_UNSUPPORTED;
    if (s->band_width != 0 && !s->same_strand) return LZGPU_NH_UNSUPPORTED;      // (the reference bands the same strand only, :844)
    if (s->n_sep1 != s->n_sep2 || s->n_sep1 == 1) return LZGPU_NH_UNSUPPORTED;
    if (s->n_sep1 && (!s->sep1 || !s->sep2)) return LZGPU_NH_UNSUPPORTED;
    for (u32 k = 0; k < s->n_sep1; k++) {                                         // ascending, inside the sequence
        if (s->sep1[k] > qlen || s->sep2[k] > qlen) return LZGPU_NH_UNSUPPORTED;
        if (k && (s->sep1[k] <= s->sep1[k - 1] || s->sep2[k] <= s->sep2[k - 1])) return LZGPU_NH_UNSUPPORTED;
    }
    // only k_count_sorted_self, k_fill_hits2<true> and k_scan_hits2<true> clip: not with bucket owners
    if (c.n_owners > 1) return LZGPU_NH_UNSUPPORTED;

    LzSelfDev sd = {};
    sd.L = (u32)c.seed.length; sd.len2 = qlen; sd.band = s->same_strand ? s->band_width : 0u;
    sd.mode = s->same_strand ? LZ_SELF_SAME : s->n_sep2 ? LZ_SELF_OPP_PARTS : LZ_SELF_OPP;
    if (sd.mode == LZ_SELF_OPP_PARTS) {
        const size_t n = (size_t)s->n_sep1;
        if ((rc = c.self_sep.ensure(2 * n * 4))) return rc;
        LZ_HIP(hipMemcpyAsync(c.self_sep.as<u32>(), s->sep1, n * 4, hipMemcpyHostToDevice, c.stream));
        LZ_HIP(hipMemcpyAsync(c.self_sep.as<u32>() + n, s->sep2, n * 4, hipMemcpyHostToDevice, c.stream));
        LZ_HIP(hipStreamSynchronize(c.stream));
        sd.sep1 = c.self_sep.as<u32>(); sd.n_sep1 = s->n_sep1;
        sd.sep2 = c.self_sep.as<u32>() + n; sd.n_sep2 = s->n_sep2;
    }
    c.self = sd;
    rc = seed_search(a, out, n_out);
    c.self = LzSelfDev{};
    return rc;
}

// Position filter (lastz --chores: hp->posFilter, filter_seed_hit_by_pos, src/seed_search.c:2269-2310, the first thing
// the hit processor does, :1072-1074).  A raw hit is kept iff its window lies inside both intervals.  The query half is
// the search interval intersected with [q_start, q_end); the target half is a constant window of hit end positions,
// [t_start + L, t_end + 1) (lz_window_self), to which the kernels that clip for a self-comparison clip every list (LZ_SELF_WINDOW).  The
// extension is not limited: the reference filters the seed, not the HSP.
extern "C" int lzgpu_seed_hit_search_within(const lz_search_args* a, const lz_pos_filter* w, lz_hsp** out, uint64_t* n_out)
{
    int rc = search_enter(a && w && out && n_out && a->sub, out, n_out); if (rc) return rc;
    LzCtx& c = g_ctx;
    if (w->t_start > w->t_end || w->q_start > w->q_end)
        return lz_fail(LZGPU_ERR_ARG, "position filter: an interval ends before it starts (target %u-%u, query %u-%u)", w->t_start, w->t_end, w->q_start, w->q_end);
    if (c.n_owners > 1) return LZGPU_NH_UNSUPPORTED;             // (the owner path has no clip)
    SeqSlot* qs; u32 qlen;                                      // (the length only: seed_search uploads a host-pointer query)
    if ((rc = lz_search_query(c, a->query, a->qlen, a->query_slot, false, qs, qlen))) return rc;
    // the search interval as ss_query reads it, then its intersection with the query interval
    const u32 lo = a->start, hi = a->end ? a->end : qlen;
    if (hi <= lo) return lz_fail(LZGPU_ERR_ARG, "in seed_hit_search(), interval is void (%u-%u)", lo, hi);
    if (hi > qlen) return lz_fail(LZGPU_ERR_ARG, "in seed_hit_search(), interval end is bad (%u>%u)", hi, qlen);
    lz_search_args b = *a;
    b.start = std::max(lo, w->q_start); b.end = std::min(hi, w->q_end);
    const u32 L = (u32)c.seed.length;
    LzSelfDev sd;
    if (b.end <= b.start || b.end - b.start < L || !lz_window_self(w->t_start, w->t_end, L, c.geom.tlen, sd)) return 0;   // no window fits: no hits, no HSPs
    c.self = sd;
    rc = seed_search(&b, out, n_out);
    c.self = LzSelfDev{};
    return rc;
}

// ------------------------------------------------------------------------------ B1 + B2 of many windows (N3)
int lzk_window_search(LzCtx& c, const LzExtendParams& P, const LzSeedDev& sd, const lz_window* wins, u32 n, const s32* score_tab_dev,
                      std::vector<lz_hsp>& out, std::vector<u32>& counts);     // window_kernels.hip

extern "C" int lzgpu_window_search(const lz_window_search_args* a, lz_hsp** out, uint64_t* n_out, uint32_t** counts)
{
    int rc = require_init(); if (rc) return rc;
    LzCtx& c = g_ctx;
    if (!a || !out || !n_out || !counts || !a->sub || !a->seed || !a->char_to_bits || (!a->windows && a->n_windows))
        return lz_fail(LZGPU_ERR_ARG, "null argument");
    *out = nullptr; *n_out = 0; *counts = nullptr;
    if (!c.target.have_raw || c.target.len != c.geom.tlen) return lz_fail(LZGPU_ERR_STATE, "no target on the device");
    LzSeedDev sd;
    if ((rc = lzh_seed_to_dev(a->seed, sd))) return rc;
    if (sd.nprobes != 1 || sd.weight > 14) return LZGPU_NH_UNSUPPORTED;
    SeqSlot* qs; u32 qlen;
    if ((rc = lz_search_query(c, a->query, a->qlen, a->query_slot, true, qs, qlen))) return rc;
    for (u32 k = 0; k < a->n_windows; k++) {
        const lz_window& w = a->windows[k];
        if (w.t_len > 20480 || w.q_len > 20480) return LZGPU_NH_UNSUPPORTED;
        if ((u64)w.t_off + w.t_len > c.target.len || (u64)w.q_off + w.q_len > qs->len) return lz_fail(LZGPU_ERR_ARG, "window %u lies outside the sequences", k);
    }
    // score classes of the (masked) matrix and the code bytes of both sequences, as for the main search
    u8 rowc[256], colc[256], cls[256]; s32 tab[LZ_NCLASS * LZ_NCLASS];
    if ((rc = lzh_score_classes(a->sub, rowc, colc, tab))) return rc;
    DevBuf& wtab = c.win_tab;
    if ((rc = wtab.ensure(sizeof(tab)))) return rc;
    LZ_HIP(hipMemcpyAsync(wtab.p, tab, sizeof(tab), hipMemcpyHostToDevice, c.stream));
    LZ_HIP(hipStreamSynchronize(c.stream));
    lzh_make_cls(rowc, a->char_to_bits, cls);
    if ((rc = slot_encode(c, c.target, cls, c.cls_t))) return rc;
    lzh_make_cls(colc, a->char_to_bits, cls);
    if ((rc = slot_encode(c, *qs, cls, c.cls_q))) return rc;
    LzExtendParams P; memset(&P, 0, sizeof(P));
    P.tcode = c.target.code_base(); P.tlen = c.target.len; P.qcode = qs->code_base(); P.qlen = qs->len;
    P.xdrop = a->xdrop; P.min_score = a->hsp_threshold; P.seed_len = (u32)sd.length;
    std::vector<lz_hsp> hs; std::vector<u32> cn;
    if ((rc = lzk_window_search(c, P, sd, a->windows, a->n_windows, wtab.as<s32>(), hs, cn))) return rc;
    lz_hsp* res = (lz_hsp*)malloc((hs.size() ? hs.size() : 1) * sizeof(lz_hsp));
    u32* cnt = (u32*)malloc((cn.size() ? cn.size() : 1) * sizeof(u32));
    if (!res || !cnt) { free(res); free(cnt); return lz_fail(LZGPU_ERR_OOM, "host malloc failed"); }
    if (!hs.empty()) memcpy(res, hs.data(), hs.size() * sizeof(lz_hsp));
    if (!cn.empty()) memcpy(cnt, cn.data(), cn.size() * sizeof(u32));
    *out = res; *n_out = hs.size(); *counts = cnt;
    return 0;
}

// ------------------------------------------------------------------------------ instrumentation

extern "C" void lzgpu_counters_reset(void) { std::lock_guard<std::mutex> lk(g_ctx.counters_m); memset(&g_ctx.counters, 0, sizeof(g_ctx.counters)); }
extern "C" int  lzgpu_counters_get(lz_counters* out) { if (!out) return LZGPU_ERR_ARG; std::lock_guard<std::mutex> lk(g_ctx.counters_m); *out = g_ctx.counters; return 0; }
extern "C" void lzgpu_profile_enable(int enable) { g_ctx.timer.enabled = g_ctx.dp_timer.enabled = enable != 0; }
extern "C" void lzgpu_profile_reset(void) { g_ctx.timer.reset(); g_ctx.dp_timer.reset(); }
extern "C" int  lzgpu_profile_get(int n, const char** name, uint64_t* launches, double* total_ms)
{
    if (n >= (int)g_ctx.timer.names.size()) n -= (int)g_ctx.timer.names.size(); else if (n >= 0) n += 0x40000000;   // the seed stage's kernels first, then B3's
    KernelTimer& t = n >= 0x40000000 ? g_ctx.timer : g_ctx.dp_timer;
    n &= 0x3FFFFFFF;
    if (n < 0 || n >= (int)t.names.size()) return 1;
    if (name) *name = t.names[n].c_str();
    if (launches) *launches = t.launches[n];
    if (total_ms) *total_ms = t.ms[n];
    return 0;
}
extern "C" int lzgpu_set_hit_capacity(uint64_t n)
{
    if (n < 1024 || n > (1ull << 31)) return LZGPU_ERR_ARG;     // hit indices inside a chunk are 32-bit
    g_ctx.hit_capacity = n; return 0;
}
extern "C" int lzgpu_set_bucket_owner(uint32_t n_owners, uint32_t owner)
{
    if (n_owners < 1 || n_owners > LZ_DIAG_SIZE || owner >= n_owners) return LZGPU_ERR_ARG;
    g_ctx.n_owners = n_owners; g_ctx.owner = owner;
    return 0;
}
extern "C" int lzgpu_set_hit_filter(const lz_hit_filter* f)
{
    g_ctx.filter_on = f != nullptr;
    if (f) g_ctx.filter = *f;
    return 0;
}
extern "C" int lzgpu_last_filter_dropped(uint64_t* dropped)
{
    if (!dropped) return LZGPU_ERR_ARG;
    *dropped = g_ctx.filter_dropped;
    return 0;
}
extern "C" int lzgpu_last_hsp_order(uint64_t* out, uint64_t n)
{
    if (!out || 2 * n != g_ctx.last_order.size()) return LZGPU_ERR_ARG;
    memcpy(out, g_ctx.last_order.data(), g_ctx.last_order.size() * 8);
    return 0;
}
extern "C" int lzgpu_last_scan_mode(void) { return g_ctx.last_scan_mode; }
extern "C" int lzgpu_set_scan_mode(int min_mode) { if (min_mode < 0 || min_mode > 2) return LZGPU_ERR_ARG; g_ctx.min_scan_mode = min_mode; return 0; }
extern "C" int lzgpu_set_hsp_capacity(uint64_t n) { if (n < 16) return LZGPU_ERR_ARG; g_ctx.hsp_capacity = n; return 0; }
