// lz_settings.hpp -- every environment switch of the library, read here and nowhere else (the rank protocol of lz_share.hip
// aside: lastz_amd/multi.py sets its four per run).  No HIP, no context: the CPU emulator of the tests compiles this too.
// tools/README.md lists the same names (tests/test_settings.py holds the two together).
//
// THE rule -- two groups:
//   LzSettings    process settings, read ONCE per process: at the first lzgpu_init in the library, at first use in a build
//                 without a context.  Read-only afterwards: any host thread reads them without a lock, and a test that
//                 varies one needs a fresh child process.
//   LzDpSwitches  per-call switches of the gapped stage, read at the top of every lzgpu_gapped_extend_batch -- before its
//                 worker threads start -- and carried by value from there: a process may flip them between two calls.
#pragma once
#include <stdlib.h>
#include <string>

struct LzSettings {
    // ---- profiling
    bool hostprof;                  // LZGPU_HOSTPROF: where the host time goes (seed search, gapped stage, big device allocations), on stderr
    bool gaps;                      // LZGPU_GAPS: idle time on a stream between two timed kernels
    std::string timer_only;         // LZGPU_TIMER_ONLY=<kernel>: time just this kernel (empty: all)
    // ---- seed stage
    int scan_mode;                  // LZGPU_SCAN_MODE=0|1|2, -1 if unset: what every lzgpu_init gives LzCtx::min_scan_mode (lzgpu_set_scan_mode)
    unsigned long long hit_capacity;    // LZGPU_HIT_CAPACITY, 0 if unset: likewise LzCtx::hit_capacity (1024 .. 2^31 hits per chunk)
    bool fused_scan;                // LZGPU_FUSED_SCAN=0: scan mode 0 on the split kernels, as modes 1 and 2, bucket owners and a too-large wctx are
    unsigned task_region_cap;       // LZGPU_TASK_REGION_CAP (tests): tiny task regions in phase A, so that hits find theirs full; 0: the rule
    // ---- gapped stage
    unsigned dp_horizon;            // LZGPU_DP_HORIZON (tests): rows a DP's pieces are worked out for at first, so that sweeps pass it; 0: the rule
    unsigned helper_min_anchors;    // LZGPU_HELPER_MIN_ANCHORS: anchors from which the commit pass gets helper threads (20000; tests: 0)
    unsigned helpers;               // LZGPU_HELPERS: how many; 0: 3, and 7 from 150 k anchors on
    unsigned batch_threads;         // LZGPU_BATCH_THREADS: host threads that work through the problems of a gapped batch (64)
    unsigned chain_threads;         // LZGPU_CHAIN_THREADS: the same for lzgpu_reduce_to_chain_batch (16)
};

struct LzDpSwitches {
    int narrow, repl;               // LZGPU_DP_NARROW, LZGPU_DP_REPL = 0|1: force the four- / two-wave kernel, the row set-up on one wave / all; -1: by the launch's size
    std::string dump;               // LZGPU_DPDUMP=<file>: one line per DP of every launch
    bool prof;                      // LZGPU_DPPROF: the longest DP of every launch, by step, on stderr
    unsigned window;                // LZGPU_DP_WINDOW: anchors speculated per round; 0: lzgpu_set_dp_window, or the default rule
};

namespace lz_env {
inline int      flag01(const char* e) { return e ? e[0] == '1' : -1; }
inline unsigned positive(const char* e, unsigned unset) { const int v = e ? atoi(e) : 0; return v > 0 ? (unsigned)v : unset; }
}

inline LzSettings lz_settings_read()
{
    using namespace lz_env;
    LzSettings s;
    s.hostprof = getenv("LZGPU_HOSTPROF") != nullptr;
    s.gaps = getenv("LZGPU_GAPS") != nullptr;
    { const char* e = getenv("LZGPU_TIMER_ONLY"); s.timer_only = e ? e : ""; }
    { const char* e = getenv("LZGPU_SCAN_MODE"); const int v = e ? atoi(e) : -1; s.scan_mode = v >= 0 && v <= 2 ? v : -1; }
    { const char* e = getenv("LZGPU_HIT_CAPACITY"); const long long v = e ? atoll(e) : 0; s.hit_capacity = v >= 1024 && v <= (1ll << 31) ? (unsigned long long)v : 0; }
    { const char* e = getenv("LZGPU_FUSED_SCAN"); s.fused_scan = !(e && atoi(e) == 0); }
    s.task_region_cap = positive(getenv("LZGPU_TASK_REGION_CAP"), 0);
    { const char* e = getenv("LZGPU_DP_HORIZON"); s.dp_horizon = (unsigned)(e ? atoi(e) : 0); }
    { const char* e = getenv("LZGPU_HELPER_MIN_ANCHORS"); s.helper_min_anchors = (unsigned)(e ? atoi(e) : 20000); }
    s.helpers = positive(getenv("LZGPU_HELPERS"), 0);
    s.batch_threads = positive(getenv("LZGPU_BATCH_THREADS"), 64);
    s.chain_threads = positive(getenv("LZGPU_CHAIN_THREADS"), 16);
    return s;
}
inline const LzSettings& lz_settings() { static const LzSettings s = lz_settings_read(); return s; }

inline LzDpSwitches lz_dp_switches()
{
    using namespace lz_env;
    LzDpSwitches d;
    d.narrow = flag01(getenv("LZGPU_DP_NARROW"));
    d.repl = flag01(getenv("LZGPU_DP_REPL"));
    { const char* e = getenv("LZGPU_DPDUMP"); d.dump = e ? e : ""; }
    d.prof = getenv("LZGPU_DPPROF") != nullptr;
    d.window = positive(getenv("LZGPU_DP_WINDOW"), 0);
    return d;
}
