// lz_ctx.hpp -- per-process device context of liblzgpu (one process per GPU).
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include <vector>
#include <map>
#include <mutex>
#include "lz_common.hpp"
#include "lz_settings.hpp"
#include "../../include/lzgpu.h"

struct DevBuf {                     // growable device allocation
    void*  p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes);       // 0 or LZGPU_ERR_OOM; contents are NOT preserved on growth
    void release();
    template <class T> T* as() const { return (T*)p; }
};

struct KernelTimer {
    struct Pending { int id; hipEvent_t a, b; hipStream_t s; };
    bool enabled = false;
    std::vector<std::string> names;
    std::vector<uint64_t> launches;
    std::vector<double> ms;
    std::vector<Pending> pending;
    std::map<hipStream_t, std::vector<hipEvent_t>> pool;   // an event is only ever recorded on one stream
    int  id_of(const char* name);
    void begin(const char* name, hipStream_t s);
    void end(hipStream_t s);
    void resolve();                 // after a stream sync: fold pending events into totals
    void reset();
    hipEvent_t get_event(hipStream_t s);
    int cur = -1; hipEvent_t cur_a = nullptr;
};

struct SeqSlot {                    // a sequence resident in HBM
    DevBuf raw;                     // LZ_SEQ_PAD + len + LZ_SEQ_PAD bytes
    DevBuf code;                    // same geometry, code bytes (see lz_common.hpp)
    DevBuf dp;                      // same geometry, DP score-class codes (unmasked scoring), B3 only
    DevBuf nib;                     // 4-bit class codes, two bases per byte (byte-code scans; built when all classes are < 8)
    bool   have_nib = false;
    DevBuf two, spc;                // 2-bit codes and the 1-bit "not A,C,G,T" mask (lz_lut.hpp), rebuilt with the codes
    DevBuf two_x, spc_x;            // the same bytes in half-overlapping 64-byte blocks (k_overlap32; read by k_scan_hits for the target)
    DevBuf mtwo, mspc;              // the match codes of an exact-match search (lz_exact.hpp): 2-bit codes and the 1-bit "matches nothing" mask, same layout as two / spc
    uint64_t match_key = 0;         // hash of the match_bits they were made from; 0 = not made / the bytes changed since
    DevBuf occ_dev;                 // [256] u32: which byte values occur
    u8     occ[256] = { 0 };        // ... on the host
    bool   has_special = false;     // some byte of the sequence is outside the 2-bit alphabet
    u32    len = 0;
    bool   have_raw = false;
    uint64_t code_key = 0;          // hash of the (class map, charToBits) the codes were built with
    uint64_t dp_key = 0;            // hash of the class map the DP codes (dp) were built with; 0 = not built / the bytes changed since
    std::vector<u8> host;           // host copy (entropy post-pass needs the raw bytes)
    u8* raw_base()  const { return raw.as<u8>()  + LZ_SEQ_PAD; }
    u8* code_base() const { return code.as<u8>() + LZ_SEQ_PAD; }
    void release()                  // every DevBuf above (a new one goes in here), and what says they hold something
    {
        DevBuf* all[] = { &raw, &code, &dp, &nib, &two, &spc, &two_x, &spc_x, &mtwo, &mspc, &occ_dev };
        for (DevBuf* b : all) b->release();
        have_raw = have_nib = false; code_key = dp_key = match_key = 0;
    }
};

struct LzCtx {
    bool inited = false;
    int  device = -1;
    int  num_cus = 256;                 // compute units of the device (MI355X: 256)
    hipStream_t stream = nullptr;
    hipStream_t dp_stream = nullptr;    // B3's own stream: lzgpu_gapped_extend(_batch) on one host thread may run beside lzgpu_seed_hit_search on another
    std::string last_error;

    // ---- target + position table (B1)
    SeqSlot target;
    bool have_table = false;
    lz_table_geom geom;
    LzSeedDev seed;
    DevBuf wstart, wpos;            // CSR table
    u64 num_words = 0;
    u64 table_gen = 0;              // counts the changes of wpos (table build, adopt, commit, a word-count limit set or lifted, a masking pass that removed entries)
    // a word-count limit in force (lzgpu_table_limit, limit_kernels.hip): wstart / wpos / num_words above are the LIMITED table the
    // searches read, and the table as it was built stands aside here; without a limit these are empty
    u32 limit = 0;                  // 0: none
    DevBuf full_wstart, full_wpos;
    u64 full_num_words = 0;
    bool limited() const { return full_wstart.p != nullptr; }    // (a limit that removes nothing keeps the table as it is: limit != 0, not limited())
    // the table as it was built, which export / geom / buffers / save / share describe whatever the searches see
    const DevBuf& built_wstart() const { return limited() ? full_wstart : wstart; }
    const DevBuf& built_wpos() const { return limited() ? full_wpos : wpos; }
    u64 built_num_words() const { return limited() ? full_num_words : num_words; }
    DevBuf wctx;                    // derived, like two_x: 32 bytes of the target's 2-bit codes per table entry (lz_lut.hpp; read by k_scan_hits2)
    u64 wctx_gen = 0; uint64_t wctx_code_key = 0;   // the table generation and the target codes wctx was built from (0: not built)

    // ---- queries
    std::map<int, SeqSlot> queries; // slot -> resident query; slot -1 = B2's transient slot (a host-pointer query), LZ_TEMP_SLOT_B3 - k = problem k of a B3 batch
                                    // that came with a host pointer (map nodes are stable: a slot's address survives other slots' insertion)
#define LZ_TEMP_SLOT_B3 (-1000)
    std::mutex slots_m;             // guards look-ups / insertions in `queries` (B2 and B3 may run on two host threads)

    // ---- seed-search scratch
    DevBuf cnt, off, pk;            // per query position: raw-hit count (u32), exclusive scan (u64), packed word (u32)
    DevBuf wiv, wsk, wsv;           // position index; (block of positions | word, position) sorted by that key (enum_kernels.hip: k_pack_words)
    DevBuf blk_start;               // where each block of positions begins in the sorted list
    std::vector<u64> blk_start_host;
    u32 blk_shift = 0, blk_count = 1;
    u64* pinned = nullptr; size_t pinned_words = 0;   // host memory the device writes small results into (no staged D2H copies)
    DevBuf bins;                    // the partition (high hash byte) of every hit of the chunk, written by the scan kernels of the unfused path
    DevBuf keys;                          // hit keys of a chunk, discovery order; on the fused path of scan mode 0
                                          // the chunk's tagged records instead (k_scan_hits2), and bins / summ are not allocated.  The partition kernels
                                          // turn it in place into the chunk's records, every tile sorted by partition (lz_tile_runs.hpp): 8 bytes per hit
    DevBuf keys2;                         // under a hit filter (lzgpu_set_hit_filter): the second key buffer the surviving keys are moved to; changes places with keys
    DevBuf filter_keep, filter_counts, filter_bases;   // ... the keep words (one bit per hit), the survivors per block of k_filter_mark and their exclusive scan
    DevBuf bin_base;                      // the 257 partition offsets (ranks)
    DevBuf hist, hist_part, run_addr;     // [tile][partition]: records, then first rank inside the block of 256 tiles; the blocks' first ranks; where the run lies
    DevBuf summ, scan_tasks, scan_ntasks; // phase A: 4-byte summary per hit of the chunk; the scans that go on past their first window
    DevBuf lut;                     // phase-A tables (lz_lut.hpp)
    DevBuf sort_tmp, scan_tmp;
    DevBuf diag_end;                // [LZ_DIAG_SIZE]
    DevBuf score_tab;               // [32*32] s32
    std::vector<s32> score_sub;     // the 256 x 256 matrix score_tab was made from (empty: none), and its row / column classes:
    u8 rowc[256] = { 0 }, colc[256] = { 0 };   // the class compression and the upload are skipped while the caller passes the same matrix
    std::vector<s32> lut_m4; s32 lut_xdrop = -1;   // likewise what lut was built from (empty: not built)
    DevBuf cls_t, cls_q, cls_tmp;   // the 256-byte class maps on the device: the target's, the query's, B3's (lz_encode_with, dp_stream)
    DevBuf win_tab;                 // the same for lzgpu_window_search (its own: the two callers may use different matrices)
    DevBuf match_tmp;               // scratch of the match-code passes (lzgpu_seed_hit_search_exact): the class map, code bytes of one sequence, presence flags
    DevBuf hsp_out, hsp_count;      // candidates + counter
    DevBuf hsp_mc;                  // [n][5]: A/C/G/T match counts of the candidates (entropy inputs) + probe index
    DevBuf dev_counters;            // u64[8]
    DevBuf tb_keys, tb_vals, tb_keys2, tb_vals2;   // table build scratch; a masking pass (mask_kernels.hip) borrows tb_keys, tb_keys2 and tb_vals2
    DevBuf mask_bits, mask_ranges;  // dynamic masking: one bit per target position 0 .. tlen, and the removal ranges of one lzgpu_table_mask call
    // ---- gapped stage (B3) and window search: device memory and settings that used to live at file scope
    // Threading: `dp` is touched on dp_stream only, by lzgpu_gapped_extend_batch's caller before its workers start and then by whichever
    // worker holds the batch rendezvous (HipDpExec::run_multi: one at a time); the win_* buffers on `stream` only, by lzgpu_window_search's caller.
    struct DpBufs { DevBuf jobs, ids, res, tab, tb, rows, ops, ops_off, ops_out, pieces, rings, sel_jobs, sel_res, problems; } dp;
    DevBuf win_jobs, win_scratch, win_out, win_count;
    bool win_attr_set = false;        // k_window_search's dynamic-LDS attribute has been set on this device context (lzgpu_shutdown clears it)
    bool settle_attr_set = false;     // likewise k_settle2's
    bool settle_exact_attr_set = false;   // likewise k_settle_exact's
    bool settle_mismatch_attr_set = false;   // ... and k_settle_mismatch's
    u64 dp_longest[4] = { 0, 0, 0, 0 };   // lzgpu_dp_longest: rows, cells, sweep and traceback ticks of the DP that swept the most rows since the last reset
    // the two settings below keep their value across shutdown + init, as hit_capacity does
    u32 dp_slot_tb = 8u << 20;        // lzgpu_set_dp_slot: the uniform traceback slot (bytes) per DP
    // Anchors speculated per round.  A launch lasts as long as its longest DP, so the fewer rounds the better: 2048 holds
    // the ~1150 anchors of a 50 Mbp strand that need a DP in one launch; a 200 Mbp strand has ~4500 (north star:
    // 7 launches, 0.73 s at 2048; 5 launches, 0.48 s at 8192 and beyond).  Default: 1/32 of the anchors, within [2048, 16384].
    u32 dp_window = 0;                // 0: the default rule; lzgpu_set_dp_window fixes it (LZGPU_DP_WINDOW, for one call, goes before either)
    u32 n_owners = 1, owner = 0;      // bucket ownership (lzgpu_set_bucket_owner)
    bool filter_on = false;           // a hit filter is in force (lzgpu_set_hit_filter); table calls do not lift it, lzgpu_shutdown does (as it resets n_owners)
    lz_hit_filter filter = {};
    u64 filter_dropped = 0;           // raw hits the last search's filter removed (lzgpu_last_filter_dropped)
    LzSelfDev self = {};              // the self-comparison filter of the search in progress (lzgpu_seed_hit_search_self) or its position filter (lzgpu_seed_hit_search_within); mode LZ_SELF_OFF otherwise
    DevBuf self_sep;                  // its separators on the device: sep1, then sep2
    std::vector<u64> last_order;      // two sort words per HSP of the last search
    int min_scan_mode = 0;            // lzgpu_set_scan_mode
    int last_scan_mode = -1;          // phase-A scan mode of the last search (0/1: look-up tables without/with special masks, 2: byte codes)
    u64 hit_capacity = (1ull << 31);    // hits per chunk (LZGPU_HIT_CAPACITY): 2^28 -> 2^30 took 10 ms off the 50 Mbp step (fewer launches, fewer passes over the sorted words), 2^30 -> 2^31 another 5.5 (a 50 Mbp strand is one chunk); the buffers follow the largest chunk: 8.1 bytes per hit on the fused path, 13.1 on the split one, 26 GiB at most
    u64 hsp_capacity = (1ull << 24);

    lz_counters counters = {};      // B2 and B3 write disjoint fields (possibly from two host threads); lzgpu_counters copies under counters_m
    std::mutex counters_m;
    KernelTimer timer;              // B1 / B2 launches (the caller's thread)
    KernelTimer dp_timer;           // B3 launches (dp_stream; possibly another host thread)

    // lzgpu_shutdown: EVERY DevBuf declared above (a new member goes in here), the slots' through SeqSlot::release, and what
    // describes their contents -- nothing outlives the device context it was made on
    void release_device_memory()
    {
        DevBuf* all[] = { &wstart, &wpos, &full_wstart, &full_wpos, &wctx, &cnt, &off, &pk, &wiv, &wsk, &wsv, &blk_start, &bins, &keys, &keys2, &filter_keep, &filter_counts, &filter_bases, &bin_base, &hist, &hist_part, &run_addr,
                          &summ, &scan_tasks, &scan_ntasks, &lut, &sort_tmp, &scan_tmp, &diag_end, &score_tab, &cls_t, &cls_q, &cls_tmp, &win_tab, &match_tmp,
                          &hsp_out, &hsp_count, &hsp_mc, &dev_counters, &tb_keys, &tb_vals, &tb_keys2, &tb_vals2, &mask_bits, &mask_ranges, &self_sep,
                          &dp.jobs, &dp.ids, &dp.res, &dp.tab, &dp.tb, &dp.rows, &dp.ops, &dp.ops_off, &dp.ops_out, &dp.pieces, &dp.rings, &dp.sel_jobs, &dp.sel_res, &dp.problems,
                          &win_jobs, &win_scratch, &win_out, &win_count };
        for (DevBuf* b : all) b->release();
        target.release();
        for (auto& kv : queries) kv.second.release();
        queries.clear();
        if (pinned) (void)hipHostFree(pinned);
        pinned = nullptr; pinned_words = 0;
        have_table = false; wctx_gen = 0; wctx_code_key = 0; limit = 0; full_num_words = 0;
        score_sub.clear(); lut_m4.clear(); lut_xdrop = -1;
        win_attr_set = false; settle_attr_set = false; settle_exact_attr_set = false; settle_mismatch_attr_set = false;
    }
};

LzCtx& lz_ctx();
int lz_bind_thread();               // brings the context up if need be and binds the CALLING thread to its device (every entry point)
int lz_fail(int code, const char* fmt, ...);
#define LZ_HIP(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) \
    return lz_fail(LZGPU_ERR_HIP, "%s:%d %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); } while (0)

// ---- the seed stage's launchers: all asynchronous on c.stream (lzk_encode: or the stream it is given).  A launcher is passed what
// varies per call -- the chunk, the kernels' parameters, the mode -- and reads the buffers that are members of LzCtx from c. ----
struct LzChunk; struct LzLutParams; struct LzExactParams; struct LzMismatchParams; struct LzFilterParams;     // lz_host.hpp, lz_lut.hpp, lz_exact.hpp, lz_filter.hpp
#include "lz_tile_runs.hpp"         // LZ_PP_TILE_HOST: hits per tile of k_partition (sizes the tile tables)
// seq_kernels.hip
int lzk_encode(LzCtx& c, const u8* raw, u8* code, u32 len, const u8* cls256_dev, hipStream_t st = nullptr, KernelTimer* timer = nullptr);   // defaults: c.stream, c.timer
int lzk_pack_nibbles(LzCtx& c, const u8* code_alloc, u8* nib, size_t nbytes);
int lzk_pack2(LzCtx& c, const u8* code_base, const u8* raw_base, u32 len, u8* two, u8* spc, u32 nmask, u32* flags256);
int lzk_overlap32(LzCtx& c, const u8* src, u8* dst, size_t nblocks);
// table_kernels.hip
int lzk_table_build(LzCtx& c);
int lzk_table_export(LzCtx& c, u32* last_dev, u32* prev_dev, u32 prev_entries);
int lzk_wctx_build(LzCtx& c);       // c.wctx (allocated by the caller) from c.wpos and c.target.two
// limit_kernels.hip (these synchronise c.stream)
void lz_limit_lift(LzCtx& c);       // c.wstart / c.wpos / c.num_words are the table as it was built again; the limited copy is released
int lzk_table_limit(LzCtx& c, u32 limit);                        // c.wstart / c.wpos -> the copy without the words of more than `limit` entries, put in their place
int lzk_table_count_distribution(LzCtx& c, std::vector<u32>& count, std::vector<u32>& words);   // the distinct list lengths > 0, ascending, and the words that have each
// mask_kernels.hip (synchronises c.stream)
int lzk_table_mask(LzCtx& c, const lz_interval* iv, u32 n, u32 tlen);   // c.wstart / c.wpos without the entries p, iv[k].start + L <= p <= iv[k].end; c.num_words, c.geom.num_words and c.table_gen follow when something went
// enum_kernels.hip (the query positions [lo, hi), n = hi - lo of them: c.cnt, c.off, c.pk, c.wiv, c.wsk, c.wsv, sized by the caller)
int lzk_count_hits(LzCtx& c, const u8* qcode, u32 lo, u32 hi);   // honours c.n_owners / c.owner and c.self
int lzk_scan_counts(LzCtx& c, u32 n);
int lzk_sample_offsets(LzCtx& c, u32 n, u32 stride, u32 ns);     // -> c.pinned
int lzk_fill_hits(LzCtx& c, u32 lo, const LzChunk& ch, u32 n);   // likewise; -> c.keys
// scan_kernels.hip
int lzk_scan_reserve(LzCtx& c, int mode, u64 max_n);
int lzk_scan_hits(LzCtx& c, int mode, const LzExtendParams& P, const LzLutParams& Q, u64 n);   // c.keys -> c.summ, and the partition byte of every hit -> c.bins
// the fused path of scan mode 0 (k_scan_hits2): enumeration + phase A in one launch, tagged records in c.keys instead of keys / summaries / partition bytes
int lzk_fused_reserve(LzCtx& c, u64 max_n);
int lzk_scan_fused(LzCtx& c, u32 lo, const LzChunk& ch, u32 n, const LzExtendParams& P, const LzLutParams& Q);
// settle_kernels.hip (n: the hits of the chunk)
int lzk_partition(LzCtx& c, bool tagged, u64 n);     // c.keys + c.summ (or tagged records in c.keys) -> records, in place; c.hist, c.run_addr
int lzk_hist_scan(LzCtx& c, u64 n);                  // after the partition of the chunk: c.hist, c.hist_part, c.bin_base
int lzk_settle(LzCtx& c, const LzExtendParams& P, u64 n, u32 out_cap);   // -> c.diag_end, c.hsp_out / c.hsp_count, c.dev_counters
int lzk_hsp_match_counts(LzCtx& c, u32 n_rec, const SeqSlot& q);         // -> c.hsp_mc
int lzk_settle_exact(LzCtx& c, const LzExactParams& P, u64 n, u32 out_cap);   // phase B of an exact-match search -> c.diag_end, c.hsp_out / c.hsp_count
int lzk_settle_mismatch(LzCtx& c, const LzMismatchParams& P, u64 n, u32 out_cap);   // phase B of an N-mismatch search, likewise
// exact_kernels.hip
int lzk_scan_exact(LzCtx& c, const LzExactParams& P, u64 n);             // phase A of an exact-match search: c.keys -> c.summ (sized by the caller)
// mismatch_kernels.hip
int lzk_scan_mismatch(LzCtx& c, const LzMismatchParams& P, u64 n);       // phase A of an N-mismatch search, likewise
// filter_kernels.hip
int lzk_filter_reserve(LzCtx& c, u64 max_n);                             // c.keys2 and the filter's scratch for chunks of up to max_n hits
int lzk_filter_hits(LzCtx& c, const LzFilterParams& F, u64 n, u64* n_kept);   // c.keys -> the keys the hit filter keeps, in order (c.keys and c.keys2 change places); synchronises c.stream
