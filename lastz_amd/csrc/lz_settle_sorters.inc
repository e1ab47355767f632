    for (u32 k = tid; k < LZ_S2_SORTW * LZ_NBIN; k += LZ_S2_TPB) (&sh.bm[0][0])[k] = 0ull;
    const bool walker = w < LZ_S2_WALKW;
    const u32 sw = w - LZ_S2_WALKW;                             // sorter wave index (sorters only)

    // ---- sorter pieces
    u64 cx[LZ_S2_ROUNDS], nx[LZ_S2_ROUNDS];                     // records of the tile to place next / to count next
    u32 cslot[LZ_S2_ROUNDS];
    // The partition's records lie in one run per partition tile (lz_tile_runs.hpp).  A sorter wave keeps a block of
    // LZ_TR_BLOCK consecutive tiles' (first rank, address) of the partition, LZ_TR_K per lane (lane l: tiles cur + K l ..),
    // that only moves forward; window_first(tt) = the first rank of the wave's window of tile tt.
    u32 cur = 0, bf[LZ_TR_K], ba[LZ_TR_K];
    auto load_block = [&]() {
#pragma unroll
        for (int j = 0; j < LZ_TR_K; j++) {
            const u32 t = cur + lane * LZ_TR_K + (u32)j;
            bf[j] = lz_tr_first(hist, hist_part, n_pp_tiles, t, part, r1);
            ba[j] = t < n_pp_tiles ? run_addr[(size_t)t * LZ_NBIN + part] : 0u;
        }
    };
    auto block_end = [&]() -> u32 { return (u32)__builtin_amdgcn_readlane((int)bf[LZ_TR_K - 1], 63); };
    auto entry_of = [&](const u32* b, u32 e) -> u32 {           // bf / ba of block entry e (wave-uniform)
        u32 v = (u32)__builtin_amdgcn_readlane((int)b[0], (int)(e / LZ_TR_K));
#pragma unroll
        for (int j = 1; j < LZ_TR_K; j++) { const u32 vj = (u32)__builtin_amdgcn_readlane((int)b[j], (int)(e / LZ_TR_K)); if (e % LZ_TR_K == (u32)j) v = vj; }
        return v;
    };
    auto window_first = [&](u32 tt) -> u32 { return r0 + tt * (u32)LZ_S2_TILE + sw * (64u * LZ_S2_ROUNDS); };
    // one step of the cursor ahead of load_tile(tt), where the loads have a whole placement to arrive (the usual tile
    // needs no more than this one: 5376 ranks are about 84 partition tiles)
    auto advance_early = [&](u32 tt) {
        if (tt < ntiles && window_first(tt) < r1 && lz_tr_block_behind(block_end(), window_first(tt))) { cur += LZ_TR_BLOCK - 1; load_block(); }
    };
    auto load_tile = [&](u32 tt, u64* x) {                      // (sorters) the wave's 448 records of tile tt, 64 per round
#pragma unroll
        for (int rr = 0; rr < LZ_S2_ROUNDS; rr++) x[rr] = ~0ull;                                    // ~0: no record
        const u32 g0 = window_first(tt);
        if (tt >= ntiles || g0 >= r1) return;                   // (wave-uniform)
        const u32 g1 = (r1 - g0 < 64u * LZ_S2_ROUNDS) ? r1 : g0 + 64u * LZ_S2_ROUNDS;
        u32 idx[LZ_S2_ROUNDS] = {};
        for (;;) {
            const u32 bend = block_end();
            if (!lz_tr_block_behind(bend, g0)) {
                // the block covers the ranks [s, lim) of the window.  Its entries ascend, so the run that holds s is a count
                // away; from there one wave-uniform cursor (entry e, its displacement, the next entry's first rank) goes
                // through the rounds, and a round's lanes at or beyond a run's first rank take that run's displacement
                // (lz_tile_runs.hpp: the entry cursor).  A round meets about one run boundary.
                const u32 bfirst = (u32)__builtin_amdgcn_readlane((int)bf[0], 0);
                const u32 s = lz_tc_start(g0, bfirst), lim = lz_tc_limit(g1, bend);
                if (s < lim) {                                  // (not so: the block's runs are all empty)
                    u32 e = ~0u;
#pragma unroll
                    for (int j = 0; j < LZ_TR_K; j++) e += (u32)__popcll(__ballot(lz_tc_at_or_below(bf[j], s)));
                    u32 nf = entry_of(bf, e + 1u);              // (e + 1 <= LZ_TR_BLOCK - 1: the bounding entry lies above s)
                    u32 dcur = lz_tr_delta(entry_of(ba, e), entry_of(bf, e));
#pragma unroll
                    for (int rr = 0; rr < LZ_S2_ROUNDS; rr++) {
                        const u32 base = g0 + (u32)rr * 64u, g = base + lane;
                        u32 d = dcur;
                        while (lz_tc_step(nf, base, lim)) {     // (stops below the bounding entry: its first rank is bend >= lim)
                            e++;
                            dcur = lz_tr_delta(entry_of(ba, e), nf);
                            if (lz_tc_take(g, nf)) d = dcur;
                            nf = entry_of(bf, e + 1u);
                        }
                        if (lz_tr_covers(g, bfirst, bend, g1)) idx[rr] = lz_tr_index(g, d);
                    }
                }
                if (bend >= g1) break;
            }
            cur += LZ_TR_BLOCK - 1; load_block();               // (a sparse partition: the window goes on in later tiles)
        }
        if (g1 - g0 == 64u * LZ_S2_ROUNDS) {                    // a full window (wave-uniform): every tile but a partition's last
#pragma unroll
            for (int rr = 0; rr < LZ_S2_ROUNDS; rr++) x[rr] = LZ_NT_LD(recs + (size_t)idx[rr]);
        } else {
#pragma unroll
            for (int rr = 0; rr < LZ_S2_ROUNDS; rr++)
                if (g0 + (u32)rr * 64u + lane < g1) x[rr] = LZ_NT_LD(recs + (size_t)idx[rr]);
        }
    };
    // count_tile / place_tile with full = true (a literal at the call: a copy without the per-round `valid` branches): every
    // lane holds a record in every round, as in all windows of all tiles but a partition's last
    auto full_window = [&](u32 tt) -> bool { return tt < ntiles && window_first(tt) < r1 && r1 - window_first(tt) >= 64u * LZ_S2_ROUNDS; };
    auto count_tile = [&](u32 tt, const u64* x, u32* slot, const bool full) {    // ranks inside (wave, bucket) -> slot[], totals -> cnt[tt & 1][sw][]
        u32* const row = sh.cnt[tt & 1u][sw];
        reinterpret_cast<uint4*>(row)[lane] = make_uint4(0u, 0u, 0u, 0u);
        u64* const bmr = sh.bm[sw];
#pragma unroll
        for (int rr = 0; rr < LZ_S2_ROUNDS; rr++) {
            const bool valid = full || x[rr] != ~0ull;
            const u32 b = LZ_REC_LOW8(x[rr]);
            if (valid) atomicOr((unsigned long long*)&bmr[b], 1ull << lane);
            const u64 peers = valid ? bmr[b] : 0ull;
            const u32 old = valid ? row[b] : 0u;
            const u32 rank = (u32)__popcll(peers & ((1ull << lane) - 1ull));
            if (valid && (peers >> lane) == 1ull) { row[b] = old + (u32)__popcll(peers); bmr[b] = 0ull; }   // the highest peer
            slot[rr] = old + rank;
        }
    };
    auto place_tile = [&](u32 tt, const u64* x, const u32* slot, const bool full) {
        // bucket bases of the tile: every sorter wave sums the 12 rows for its own use (lane l: buckets 4l .. 4l+3)
        const u32 (*cn)[LZ_NBIN] = sh.cnt[tt & 1u];
        uint4 tot = make_uint4(0u, 0u, 0u, 0u), pre = tot;
#pragma unroll
        for (u32 k = 0; k < LZ_S2_SORTW; k++) {
            const uint4 v = reinterpret_cast<const uint4*>(cn[k])[lane];
            if (k == sw) pre = tot;
            tot.x += v.x; tot.y += v.y; tot.z += v.z; tot.w += v.w;
        }
        const u32 mine = tot.x + tot.y + tot.z + tot.w;
        u32 inc = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const u32 t = __shfl_up(inc, d); if ((int)lane >= d) inc += t; }
        const u32 b0 = inc - mine, b1 = b0 + tot.x, b2 = b1 + tot.y, b3 = b2 + tot.z;
        reinterpret_cast<uint4*>(sh.woff[sw])[lane] = make_uint4(b0 + pre.x, b1 + pre.y, b2 + pre.z, b3 + pre.w);
        if (sw == 0) {
            reinterpret_cast<uint4*>(sh.lbeg[tt & 1u])[lane] = make_uint4(b0, b1, b2, b3);
            reinterpret_cast<uint4*>(sh.lcnt[tt & 1u])[lane] = tot;
        }
        u64* const dst = sh.rec[tt & 1u];
#pragma unroll
        for (int rr = 0; rr < LZ_S2_ROUNDS; rr++)
            if (full || x[rr] != ~0ull) dst[sh.woff[sw][LZ_REC_LOW8(x[rr])] + slot[rr]] = x[rr];
    };

    // ---- the two roles run their own loops (the register allocator sees two disjoint sets of live values) and
    // meet at the same barriers: 3 in the prologue, one per tile.  (s_barrier counts arrivals per wave, not places.)
    __syncthreads();                                            // tab, bm
    if (!walker) {
        // prologue: tile 0 counted | tile 0 placed, tile 1 counted | then per interval t: tile t+1 placed, tile t+2 counted
        load_block();
        load_tile(0, cx); load_tile(1, nx); count_tile(0, cx, cslot, false);
        __syncthreads();
        place_tile(0, cx, cslot, false);
#pragma unroll
        for (int rr = 0; rr < LZ_S2_ROUNDS; rr++) cx[rr] = nx[rr];
        load_tile(2, nx);
        count_tile(1, cx, cslot, false);
        __syncthreads();
        for (u32 t = 0; t < ntiles; t++) {
            LZ_S2_CLK_BEGIN(sw == 0 && lane == 0);
            advance_early(t + 3);
            if (full_window(t + 1)) place_tile(t + 1, cx, cslot, true); else if (t + 1 < ntiles) place_tile(t + 1, cx, cslot, false);
#pragma unroll
            for (int rr = 0; rr < LZ_S2_ROUNDS; rr++) cx[rr] = nx[rr];
            load_tile(t + 3, nx);                               // (past the last tile: no loads, "no record")
            if (full_window(t + 2)) count_tile(t + 2, cx, cslot, true); else if (t + 2 < ntiles) count_tile(t + 2, cx, cslot, false);
            LZ_S2_CLK_MID(sw == 0 && lane == 0, 2);
            __syncthreads();
            LZ_S2_CLK_END(sw == 0 && lane == 0, 3);
        }
        return;
    }
    __syncthreads();
    __syncthreads();
