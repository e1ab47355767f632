// lz_enum_lists.inc -- the lists of one probe group of one query position: a fragment of text, included inside a loop over the
// position's probe groups.  Plain C++ (no wave intrinsic, nothing of the HIP runtime): it compiles for the device and for the host.
//   expects   sd (LzSeedDev), r (the group's first probe, a multiple of LZ_FILL_GROUP), w_l (the position's packed seed word),
//             in (the position takes part), wstart, wpos (the position table, CSR), SELF (compile-time: the lists are clipped)
//             and, read only if SELF, slo, shi (lz_self_bounds of the position)
//   defines   la[p], len[p]  first wpos index and length of the list of probe r + p (length 0: no such probe, or !in),
//             total          the sum of the lengths
//   included  by lz_enum_place.inc (k_fill_hits2, k_scan_hits2) and, for their cnt_grp, by tests/emul/emul_self.cpp and
//             tests/emul/emul_pos_filter.cpp: the CPU tests of the clip run these lines, not a restatement of them.
// Every load of the group is issued before the first is used (13 independent pairs in flight per lane for the default seed): a
// lane without a probe reads word 0's bounds and drops them.  k_count_sorted_self (enum_kernels.hip) states the same loop for itself.
u32 la[LZ_FILL_GROUP], len[LZ_FILL_GROUP]; u32 total = 0;
#pragma unroll
for (int p = 0; p < LZ_FILL_GROUP; p++) {
    const bool on = in && r + p < sd.nprobes;
    const u32 w = on ? (w_l ^ sd.probe_xor[(r + p) & (LZ_MAX_PROBES - 1)]) : 0u;
    la[p] = wstart[w]; len[p] = wstart[w + 1];
}
#pragma unroll
for (int p = 0; p < LZ_FILL_GROUP; p++) {
    const bool on = in && r + p < sd.nprobes;
    len[p] = on ? len[p] - la[p] : 0u;
    if (!SELF) total += len[p];
}
if (SELF) {
    lz_clip_runs<LZ_FILL_GROUP>(wpos, la, len, slo, shi);
#pragma unroll
    for (int p = 0; p < LZ_FILL_GROUP; p++) total += len[p];
}
