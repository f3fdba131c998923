// Rows by id, their rank, the entry at a rank, range search and removal (hac_index_reconstruct*, hac_index_score_ids*,
// hac_index_rank_ids*, hac_index_count_ahead_device, hac_index_entries_at*, hac_index_range_search*, hac_index_remove_ids): everything
// between the C ABI and the kernels of flat_ip.hip ("rows by id"), rank.inc, at_rank.inc, range.inc and remove.inc.  Included by flat_ip.hip behind hac_index; free functions
// over one shard (DeviceIndex &), which lends its segment table, its stream, its pinned slab, its staging buffers and the
// workspaces ws_q / ws_ids / ws_D / ws_I / ws_rank / ws_atrank / ws_range -- nothing of the search state (remove_rows_shard alone changes
// the segments).  The searches that return top-k keys are search_host.inc's, which follows and uses the helpers here.
namespace {

// ---- device forms: enqueue on `st` and return.  The only wait is the segment table's upload after an add / reset / a changed
// image, which the first search pays too; nothing is read back or written to the status ring, so once the table is up (and,
// for the rank calls, the workspace of the largest shape exists) these calls can be captured into a graph.
int check_dev_ptr(const void *p, const char *what) {
    if (((uintptr_t)p & 15) != 0) return fail(HAC_ERR_INVALID, "%s: device pointer must be 16-byte aligned", what);
    return HAC_OK;
}
int rows_range_device(DeviceIndex &x, int64_t i0, int64_t n, float *out_dev, hipStream_t st) {
    if (i0 < 0 || n < 0 || i0 > x.ntotal || n > x.ntotal - i0)
        return fail(HAC_ERR_INVALID, "reconstruct: rows [%lld, %lld + %lld) are not inside [0, %lld]", (long long)i0, (long long)i0, (long long)n, (long long)x.ntotal);
    if (n == 0) return HAC_OK;
    HAC_TRY(check_dev_ptr(out_dev, "reconstruct"));
    HAC_TRY(x.upload_segs(st));
    const long g_lo = (long)(i0 / GROUP_ROWS), g_hi = (long)((i0 + n + GROUP_ROWS - 1) / GROUP_ROWS);
    untile_range_kernel<<<dim3((unsigned)(g_hi - g_lo)), dim3(256), 0, st>>>(x.d_segs, x.nseg_live, (long)i0, (long)n, x.K4, reinterpret_cast<f4 *>(out_dev));
    HAC_HIP(hipGetLastError());
    return HAC_OK;
}
int rows_ids_device(DeviceIndex &x, const int64_t *ids_dev, int64_t n, float *out_dev, hipStream_t st) {
    if (n == 0) return HAC_OK;
    if (n > (int64_t)0x7FFFFFFF * (4 * ROWS_PER_WAVE)) return fail(HAC_ERR_UNSUPPORTED, "reconstruct: %lld ids in one call exceed the grid", (long long)n);
    HAC_TRY(check_dev_ptr(out_dev, "reconstruct"));
    HAC_TRY(x.upload_segs(st));
    const int64_t per_wg = 4 * ROWS_PER_WAVE;
    rows_by_id_kernel<<<dim3((unsigned)((n + per_wg - 1) / per_wg)), dim3(256), 0, st>>>(x.d_segs, x.d_rimg, x.nseg_live, (const long long *)ids_dev, (long)n,
                                                                                       (long)x.ntotal, x.K4, reinterpret_cast<f4 *>(out_dev));
    HAC_HIP(hipGetLastError());
    return HAC_OK;
}
int score_ids_device(DeviceIndex &x, const float *q_dev, int64_t nq, const int64_t *ids_dev, int64_t m, float *D_dev, hipStream_t st) {
    if (nq == 0 || m == 0) return HAC_OK;
    const int64_t bpq = (m + 255) / 256;
    if (bpq > 0x7FFFFFFF / nq) return fail(HAC_ERR_UNSUPPORTED, "score_ids: %lld x %lld pairs in one call exceed the grid", (long long)nq, (long long)m);
    HAC_TRY(check_dev_ptr(q_dev, "score_ids"));
    HAC_TRY(x.upload_segs(st));
    score_ids_kernel<<<dim3((unsigned)(nq * bpq)), dim3(256), 0, st>>>(x.d_segs, x.d_rimg, x.nseg_live, q_dev, (const long long *)ids_dev, (long)m, (u32)bpq,
                                                                      (long)x.ntotal, x.K4, D_dev);
    HAC_HIP(hipGetLastError());
    return HAC_OK;
}

// The rank calls need a workspace (the counters and, for rank_ids, the reference scores: nq * m * 12 bytes), which grows by
// the rule of the search workspaces.
int check_rank_size(const char *what, int64_t nq, int64_t m) {
    if (m > ((int64_t)1 << 40) / nq) return fail(HAC_ERR_UNSUPPORTED, "%s: %lld x %lld pairs in one call exceed the workspace", what, (long long)nq, (long long)m);
    return HAC_OK;
}
u64 *rank_counters(const DeviceIndex &x) { return (u64 *)x.ws_rank.p; }
float *rank_scores(const DeviceIndex &x, int64_t nq, int64_t m) { return (float *)((u64 *)x.ws_rank.p + (size_t)nq * m); }
// out[i][j] = count_ahead(q[i], ref_score[i][j], ref_bound[i][j]) over this shard's rows, or -1 (rank_finish_kernel)
int count_ahead_device(DeviceIndex &x, const char *what, const float *q_dev, int64_t nq, const float *ref_score_dev, const int64_t *ref_bound_dev,
                       bool bounds_are_ids, int64_t m, int64_t *out_dev, hipStream_t st) {
    if (nq == 0 || m == 0) return HAC_OK;
    HAC_TRY(check_rank_size(what, nq, m));
    HAC_TRY(check_dev_ptr(q_dev, what));
    HAC_TRY(x.ws_rank.reserve((size_t)nq * m * 12));
    HAC_TRY(x.upload_segs(st));
    HAC_HIP(hipMemsetAsync(rank_counters(x), 0, (size_t)nq * m * 8, st));
    const u32 G = (u32)((x.ntotal + GROUP_ROWS - 1) / GROUP_ROWS);
    const int64_t chunks = (m + RANK_MT - 1) / RANK_MT;
    // queries in chunks of QUERY_CHUNK, as the exact search takes them; grid.x as make_plan sizes scan16's for the same rows and queries
    for (int64_t off = 0; off < nq && G > 0; off += DeviceIndex::QUERY_CHUNK) {
        const int64_t n = std::min<int64_t>(DeviceIndex::QUERY_CHUNK, nq - off);
        ScanArgs a = x.scan_args(q_dev + (size_t)off * x.d, n);
        a.QT = (int)std::min<int64_t>(16, n);
        a.n_items = G;
        const int T = (int)((n + a.QT - 1) / a.QT);
        const size_t lds = rank_lds(x.K4, a.QT, RANK_MT);
        // resident workgroups per CU: LDS-limited like scan16's, and 3 by the kernel's registers (144 of 512 per SIMD, one wave of a workgroup each)
        const long P = x.row_streams(lds, SCAN_WAVES, 3, T, G, 0);
        RankArgs ra{ref_score_dev + (size_t)off * m, (const long long *)ref_bound_dev + (size_t)off * m, rank_counters(x) + (size_t)off * m, (long)m, 0u};
        for (int64_t c0 = 0; c0 < chunks; c0 += 65535) {
            ra.chunk0 = (u32)c0;
            const unsigned nz = (unsigned)std::min<int64_t>(65535, chunks - c0);
            count_ahead_kernel<RANK_MT><<<dim3((unsigned)P, (unsigned)T, nz), dim3(SCAN_WAVES * 64), lds, st>>>(a, ra);
            HAC_HIP(hipGetLastError());
        }
        snprintf(x.last_plan, sizeof x.last_plan, "count_ahead_kernel<MT=%d> grid=(%ld,%d) QT=%d chunks=%lld lds=%zu", RANK_MT, P, T, a.QT, (long long)chunks, lds);
        x.plan_text_slot = -1;
    }
    const int64_t total = nq * m;
    rank_finish_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st>>>(rank_counters(x), ref_score_dev, (const long long *)ref_bound_dev, bounds_are_ids,
                                                                                   (long)total, (long)x.ntotal, (long long *)out_dev);
    HAC_HIP(hipGetLastError());
    return HAC_OK;
}
// rank[i][j] = count_ahead(q[i], score_ids(q[i], ids[i][j]), ids[i][j]): score_ids_kernel into the workspace, the counters, the finish
int rank_ids_device(DeviceIndex &x, const float *q_dev, int64_t nq, const int64_t *ids_dev, int64_t m, int64_t *rank_dev, hipStream_t st) {
    if (nq == 0 || m == 0) return HAC_OK;
    HAC_TRY(check_rank_size("rank_ids", nq, m));
    HAC_TRY(x.ws_rank.reserve((size_t)nq * m * 12));
    HAC_TRY(score_ids_device(x, q_dev, nq, ids_dev, m, rank_scores(x, nq, m), st));
    return count_ahead_device(x, "rank_ids", q_dev, nq, rank_scores(x, nq, m), ids_dev, true, m, rank_dev, st);
}

// ---- entry at a rank (at_rank.inc).  The digits a selection runs over: every score digit, and the position digits from the
// highest one in which two rows of the index can differ -- the low key words of positions pos_base .. pos_base + ntotal - 1 are
// consecutive, so the digits above the highest bit in which the first and the last differ are the same for every row and go
// into the prefix from the start (const_bits).  passes = 32 / BITS + ceil(bit_length(pos_base ^ (pos_base + ntotal - 1)) / BITS).
struct AtDigits { int passes; u64 const_bits; };
AtDigits at_rank_digits(u32 pos_base, int64_t ntotal) {
    const u32 lo_first = 0xFFFFFFFFu - pos_base, lo_last = 0xFFFFFFFFu - (u32)(pos_base + (u64)ntotal - 1);
    int bits = 0;
    for (u32 v = lo_first ^ lo_last; v; v >>= 1) ++bits;
    const int npos = (bits + AT_BITS - 1) / AT_BITS;
    const u64 mask = npos * AT_BITS >= 32 ? 0ull : (0xFFFFFFFFull >> (npos * AT_BITS)) << (npos * AT_BITS);
    return AtDigits{32 / AT_BITS + npos, (u64)lo_first & mask};
}
// The workspace of one call: a launch's pair states and histograms (reused by the next launch, in stream order), then -- the
// forms that return D / I -- the call's keys.  It grows by the rule of the search workspaces.
constexpr int64_t AT_LAUNCH_PAIRS = DeviceIndex::QUERY_CHUNK;
constexpr size_t AT_PAIR_BYTES = sizeof(AtState) + ((size_t)4 << AT_BITS);
// keys_out[i][j] = entry_at(q[i], ranks[i][j]) as a packed key in the position space of pos_base, 0 = padding (a rank outside
// [0, |L(q[i])|)); keys_out == null: into the workspace (*keys_ws)
int entries_at_keys_device(DeviceIndex &x, const char *what, const float *q_dev, int64_t nq, const int64_t *ranks_dev, int64_t m, u64 *keys_out, u32 pos_base,
                           hipStream_t st, u64 **keys_ws = nullptr) {
    if (nq == 0 || m == 0) return HAC_OK;
    HAC_TRY(check_rank_size(what, nq, m));
    if (m > ((int64_t)1 << 38) / nq) return fail(HAC_ERR_UNSUPPORTED, "%s: %lld x %lld pairs in one call exceed the grid", what, (long long)nq, (long long)m);
    HAC_TRY(check_dev_ptr(q_dev, what));
    if ((uint64_t)pos_base + (uint64_t)x.ntotal > 0xFFFFFFFFull) return fail(HAC_ERR_UNSUPPORTED, "row positions exceed 32 bits");
    const int64_t N = nq * m;
    const int QT = (int)std::min<int64_t>(16, N);
    const int64_t tiles_all = (N + QT - 1) / QT;
    int64_t TL = AT_LAUNCH_PAIRS / 16;
    if (x.tune.debug_at_rank_tiles > 0) TL = std::min<int64_t>(TL, x.tune.debug_at_rank_tiles);
    TL = std::min(TL, tiles_all);
    const int64_t PL = std::min(N, TL * QT);   // pairs per launch
    HAC_TRY(x.ws_atrank.reserve((size_t)PL * AT_PAIR_BYTES + (keys_out ? 0 : (size_t)N * 8)));
    AtState *state = (AtState *)x.ws_atrank.p;
    u32 *hist = (u32 *)(state + PL);
    if (!keys_out) *keys_ws = keys_out = (u64 *)(hist + ((size_t)PL << AT_BITS));
    if (x.ntotal == 0) {
        HAC_HIP(hipMemsetAsync(keys_out, 0, (size_t)N * 8, st));
        return HAC_OK;
    }
    HAC_TRY(x.upload_segs(st));
    HAC_HIP(hipMemsetAsync(hist, 0, (size_t)PL * 4 << AT_BITS, st));
    const u32 G = (u32)((x.ntotal + GROUP_ROWS - 1) / GROUP_ROWS);
    const AtDigits dg = at_rank_digits(pos_base, x.ntotal);
    for (int64_t off = 0; off < N; off += PL) {
        const int64_t n = std::min(PL, N - off);
        ScanArgs a = x.scan_args(q_dev, n);   // (the queries of the whole call: a pair finds its own)
        a.QT = (int)std::min<int64_t>(16, n);
        a.n_items = G;
        a.pos_base = pos_base;
        const int T = (int)((n + a.QT - 1) / a.QT);
        const size_t lds = at_rank_lds(x.K4, a.QT, AT_BITS);
        // resident workgroups per CU: LDS-limited, and 3 by the kernel's registers, as count_ahead_kernel
        const long P = x.row_streams(lds, SCAN_WAVES, 3, T, G, x.tune.at_rank_p);
        AtArgs ra{state, hist, (long)m, (long)off, 0};
        for (int p = 0; p < dg.passes; ++p) {
            // the score digits from the top, then the position digits that can differ, down to bit 0
            ra.shift = p < 32 / AT_BITS ? 64 - AT_BITS * (p + 1) : AT_BITS * (dg.passes - 1 - p);
            HAC_TRY(x.prof_begin(st));   // (hac_index_set_profiling: every pass is a timed scan, in launch order)
            rank_hist_kernel<AT_BITS><<<dim3((unsigned)P, (unsigned)T), dim3(SCAN_WAVES * 64), lds, st>>>(a, ra);
            HAC_HIP(hipGetLastError());
            HAC_TRY(x.prof_end(st));
            rank_narrow_kernel<AT_BITS><<<dim3((unsigned)n), dim3(64), 0, st>>>(hist, state, (const long long *)ranks_dev + off, ra.shift, dg.const_bits,
                                                                               p == dg.passes - 1 ? keys_out + off : nullptr);
            HAC_HIP(hipGetLastError());
        }
        if (off == 0) {
            snprintf(x.last_plan, sizeof x.last_plan, "rank_hist_kernel<BITS=%d> grid=(%ld,%d) QT=%d passes=%d lds=%zu", AT_BITS, P, T, a.QT, dg.passes, lds);
            x.plan_text_slot = -1;
        }
    }
    return HAC_OK;
}
// (D, I)[i][j] = entry_at(q[i], ranks[i][j]): the keys into the workspace, then keys_to_results_kernel, with or without id_map
int entries_at_device(DeviceIndex &x, const float *q_dev, int64_t nq, const int64_t *ranks_dev, int64_t m, float *D_dev, int64_t *I_dev,
                      const int64_t *id_map_dev, hipStream_t st) {
    if (nq == 0 || m == 0) return HAC_OK;
    u64 *keys = nullptr;
    HAC_TRY(entries_at_keys_device(x, "entries_at_device", q_dev, nq, ranks_dev, m, nullptr, 0u, st, &keys));
    const int64_t N = nq * m;
    keys_to_results_kernel<<<dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st>>>(keys, (long)N, (const long long *)id_map_dev, D_dev, (long long *)I_dev);
    HAC_HIP(hipGetLastError());
    return HAC_OK;
}

// ---- range search (range.inc).  The workspace of one call of (nq, cap): control words, counters, lims, the two key buffers
// (the staged keys share the second one: the scatter has read them before the sort or a merge pass writes there), then the
// u32 planes.  20 bytes per result of capacity; it grows by the rule of the search workspaces.
struct RangeWs {
    u64 *ctl, *counts;
    long long *lims;
    u64 *buf[2];
    u32 *blk, *qcur, *stage_q;
    static size_t bytes(int64_t nq, int64_t cap) { return ((size_t)RANGE_CTL_WORDS + 2 * nq + 1 + 2 * cap) * 8 + ((size_t)2 * nq + 1 + cap) * 4; }
    RangeWs(void *p, int64_t nq, int64_t cap) {
        ctl = (u64 *)p;
        counts = ctl + RANGE_CTL_WORDS;
        lims = (long long *)(counts + nq);
        buf[0] = (u64 *)(lims + nq + 1);
        buf[1] = buf[0] + cap;
        blk = (u32 *)(buf[1] + cap);
        qcur = blk + nq + 1;
        stage_q = qcur + nq;
    }
};
// merge passes that sort a segment of up to cap keys out of LDS-sorted blocks: ceil(log2(ceil(cap / RANGE_SORT_N)))
int range_merge_passes(int64_t cap) {
    int p = 0;
    for (int64_t blocks = (cap + RANGE_SORT_N - 1) / RANGE_SORT_N; ((int64_t)1 << p) < blocks; ++p) {}
    return p;
}
// the capacity the workspace is sized for: no more results than (query, row) pairs, so a generous cap costs nothing
int64_t range_cap(const DeviceIndex &x, int64_t nq, int64_t cap) {
    return x.ntotal == 0 ? 0 : (nq > INT64_MAX / x.ntotal ? cap : std::min<int64_t>(cap, nq * x.ntotal));
}
// Everything of a range search that runs on the device, enqueued on `st` (nq > 0, cap >= 0): lims (lims_dev, or the workspace's
// own when null) is always complete; if the total fits cap, the sorted keys of all queries are in *keys_out, segment by segment,
// and -- with D_dev -- the results in D_dev / I_dev.  The launches depend on (nq, cap) and the index's size only.
int range_device(DeviceIndex &x, const char *what, const float *q_dev, int64_t nq, const float *radius_dev, int64_t cap, int64_t *lims_dev, float *D_dev,
                 int64_t *I_dev, const int64_t *id_map_dev, hipStream_t st, const u64 **keys_out = nullptr) {
    const int64_t cap_eff = range_cap(x, nq, cap);
    if (nq > ((int64_t)1 << 30) || cap_eff > ((int64_t)1 << 38))
        return fail(HAC_ERR_UNSUPPORTED, "%s: %lld queries with room for %lld results in one call exceed the grid", what, (long long)nq, (long long)cap_eff);
    HAC_TRY(check_dev_ptr(q_dev, what));
    HAC_TRY(x.ws_range.reserve(RangeWs::bytes(nq, cap_eff)));
    const RangeWs ws(x.ws_range.p, nq, cap_eff);
    if (!lims_dev) lims_dev = (int64_t *)ws.lims;
    HAC_TRY(x.upload_segs(st));
    HAC_HIP(hipMemsetAsync(ws.ctl, 0, (size_t)(RANGE_CTL_WORDS + nq) * 8, st));
    const u32 G = (u32)((x.ntotal + GROUP_ROWS - 1) / GROUP_ROWS);
    long P = 0;
    int T = 0, QT = (int)std::min<int64_t>(16, nq);
    size_t lds = range_lds(x.K4, QT);
    // queries in chunks of QUERY_CHUNK, the grid as count_ahead_device sizes count_ahead_kernel's for the same rows and queries
    for (int64_t off = 0; off < nq && G > 0; off += DeviceIndex::QUERY_CHUNK) {
        const int64_t n = std::min<int64_t>(DeviceIndex::QUERY_CHUNK, nq - off);
        ScanArgs a = x.scan_args(q_dev + (size_t)off * x.d, n);
        a.QT = QT = (int)std::min<int64_t>(16, n);
        a.n_items = G;
        T = (int)((n + a.QT - 1) / a.QT);
        lds = range_lds(x.K4, a.QT);
        P = x.row_streams(lds, SCAN_WAVES, 3, T, G, 0);   // (3 workgroups per CU at most, as count_ahead_kernel: the same registers)
        const RangeArgs ra{radius_dev + off, ws.counts + off, ws.ctl + RANGE_CURSOR, ws.buf[1], ws.stage_q, (u64)cap_eff, (u32)off};
        range_emit_kernel<<<dim3((unsigned)P, (unsigned)T), dim3(SCAN_WAVES * 64), lds, st>>>(a, ra);
        HAC_HIP(hipGetLastError());
    }
    range_offsets_kernel<<<dim3(1), dim3(RANGE_THREADS), 0, st>>>(ws.counts, (long)nq, (u64)cap, ws.ctl, (long long *)lims_dev, ws.blk, ws.qcur);
    HAC_HIP(hipGetLastError());
    const int passes = range_merge_passes(cap_eff);
    if (cap_eff > 0) {
        const unsigned per_key = (unsigned)((cap_eff + RANGE_THREADS - 1) / RANGE_THREADS);
        // a segment's blocks: floor(len / N) full ones and at most one more per query
        const unsigned blocks = (unsigned)(cap_eff / RANGE_SORT_N + std::min<int64_t>(nq, cap_eff));
        range_scatter_kernel<<<dim3(per_key), dim3(RANGE_THREADS), 0, st>>>(ws.ctl, ws.buf[1], ws.stage_q, (const long long *)lims_dev, ws.qcur, ws.buf[0]);
        HAC_HIP(hipGetLastError());
        range_sort_kernel<<<dim3(blocks), dim3(RANGE_THREADS), 0, st>>>(ws.ctl, (const long long *)lims_dev, ws.blk, (long)nq, passes, ws.buf[0], ws.buf[1]);
        HAC_HIP(hipGetLastError());
        for (int p = 0; p < passes; ++p) {
            range_merge_kernel<<<dim3(blocks), dim3(RANGE_THREADS), 0, st>>>(ws.ctl, (const long long *)lims_dev, ws.blk, (long)nq, passes, p, ws.buf[p & 1],
                                                                            ws.buf[(p + 1) & 1]);
            HAC_HIP(hipGetLastError());
        }
        if (D_dev) {
            range_results_kernel<<<dim3(per_key), dim3(RANGE_THREADS), 0, st>>>(ws.ctl, ws.buf[passes & 1], (const long long *)id_map_dev, D_dev, (long long *)I_dev);
            HAC_HIP(hipGetLastError());
        }
    }
    if (keys_out) *keys_out = ws.buf[passes & 1];
    snprintf(x.last_plan, sizeof x.last_plan, "range_emit_kernel grid=(%ld,%d) QT=%d cap=%lld sort_lds=%d merge_passes=%d lds=%zu", P, T, QT, (long long)cap,
             RANGE_SORT_N, passes, lds);
    x.plan_text_slot = -1;
    return HAC_OK;
}

// ---- host forms over one shard's rows: synchronous, on the shard's own stream, one chunk in flight.  They run on
// for_each_shard's threads, so they touch the shard's own buffers only and write disjoint slots of the caller's output.
// `bytes` of the shard's pinned slab, free to be written: it may still be the source of an earlier copy on the shard's stream.
int pin_slab(DeviceIndex &x, size_t bytes, char *&slab) {
    HAC_TRY(x.pin_reserve(bytes));
    HAC_HIP(hipStreamSynchronize(x.stream));
    slab = static_cast<char *>(x.h_pin.p);
    return HAC_OK;
}

// Rows, staged through the add's 64-MiB buffers a chunk at a time (the whole of a 25M-row index is 77 GB: it never exists on
// the device a second time).  ids != null: out row pos[i] (or i) = row ids[i], local numbering, < 0 = all-ones; ids == null:
// the rows [i0, i0 + n).
int read_rows_host(DeviceIndex &x, const int64_t *ids, const int64_t *pos, int64_t i0, int64_t n, float *out) {
    if (n == 0) return HAC_OK;
    DeviceGuard g(x.device);
    if (!g.ok) return fail(HAC_ERR_HIP, "cannot select HIP device %d", x.device);
    const int64_t chunk_rows = x.stage_rows();
    const size_t row_bytes = (size_t)x.d * 4, id_bytes = ids ? (size_t)std::min(chunk_rows, n) * 8 : 0;
    HAC_TRY(x.stage_reserve());
    HAC_TRY(x.ws_ids.reserve(id_bytes));
    char *hi = nullptr;
    HAC_TRY(pin_slab(x, id_bytes, hi));
    for (int64_t done = 0; done < n; done += chunk_rows) {
        const int64_t m = std::min(chunk_rows, n - done);
        if (ids) {
            std::memcpy(hi, ids + done, (size_t)m * 8);
            HAC_HIP(hipMemcpyAsync(x.ws_ids.p, hi, (size_t)m * 8, hipMemcpyHostToDevice, x.stream));
            HAC_TRY(rows_ids_device(x, (const int64_t *)x.ws_ids.p, m, (float *)x.ws_stage[0].p, x.stream));
        } else {
            HAC_TRY(rows_range_device(x, i0 + done, m, (float *)x.ws_stage[0].p, x.stream));
        }
        HAC_HIP(hipMemcpyAsync(x.h_stage[0].p, x.ws_stage[0].p, (size_t)m * row_bytes, hipMemcpyDeviceToHost, x.stream));
        HAC_HIP(hipStreamSynchronize(x.stream));
        const char *src = static_cast<const char *>(x.h_stage[0].p);
        if (pos) {
            for (int64_t i = 0; i < m; ++i) std::memcpy(out + (size_t)pos[done + i] * x.d, src + (size_t)i * row_bytes, row_bytes);
        } else {
            std::memcpy(out + (size_t)done * x.d, src, (size_t)m * row_bytes);
        }
    }
    return HAC_OK;
}

// One input plane of a host matrix [nq][m] of (query, row) pairs: `width` bytes per pair, staged into `dev`.  host == null: the
// device form fills the plane itself; it still counts towards the chunk's size.
struct PairPlane { const void *host; size_t width; GrowBuf *dev; };
// out[i][j] = what launch(nqc, mc) leaves in out_dev for the pair (q[i], planes[.][i][j]), for all of a host matrix: chunked over
// the queries and, for very long lists, over j, so that one chunk's queries, planes and results fit ~64 MiB (QC x MC pairs,
// MC = min(m, 2^20)).  launch enqueues the device form on the shard's stream: queries in ws_q, planes and results [nqc][mc].
// planes[0] holds the ids; with has_skip, pairs whose id == skip are another shard's and their slots of `out` are left alone.
template <class Out, size_t NP, class Launch>
int pair_matrix_host(DeviceIndex &x, const float *q, int64_t nq, int64_t m, const PairPlane (&planes)[NP], Out *out, GrowBuf &out_dev, bool has_skip,
                     int64_t skip, Launch launch) {
    if (nq == 0 || m == 0) return HAC_OK;
    DeviceGuard g(x.device);
    if (!g.ok) return fail(HAC_ERR_HIP, "cannot select HIP device %d", x.device);
    size_t pair_bytes = sizeof(Out);
    for (const PairPlane &p : planes) pair_bytes += p.width;
    const size_t budget = (size_t)64 << 20, q_bytes = (size_t)x.d * 4;
    const int64_t MC = std::min<int64_t>(m, 1 << 20);
    const int64_t QC = std::max<int64_t>(1, std::min<int64_t>(nq, (int64_t)(budget / ((size_t)MC * pair_bytes + q_bytes))));
    const size_t pairs = (size_t)QC * MC;
    HAC_TRY(x.ws_q.reserve(QC * q_bytes));
    for (const PairPlane &p : planes) HAC_TRY(p.dev->reserve(pairs * p.width));
    HAC_TRY(out_dev.reserve(pairs * sizeof(Out)));
    char *hq = nullptr, *hp[NP];   // the slab: queries, results, planes
    HAC_TRY(pin_slab(x, QC * q_bytes + pairs * pair_bytes, hq));
    Out *res = reinterpret_cast<Out *>(hq + QC * q_bytes);
    hp[0] = reinterpret_cast<char *>(res + pairs);
    for (size_t p = 1; p < NP; ++p) hp[p] = hp[p - 1] + pairs * planes[p - 1].width;
    const int64_t *ids = static_cast<const int64_t *>(planes[0].host);
    for (int64_t q0 = 0; q0 < nq; q0 += QC) {
        const int64_t nqc = std::min(QC, nq - q0);
        std::memcpy(hq, q + (size_t)q0 * x.d, nqc * q_bytes);
        HAC_HIP(hipMemcpyAsync(x.ws_q.p, hq, nqc * q_bytes, hipMemcpyHostToDevice, x.stream));
        for (int64_t j0 = 0; j0 < m; j0 += MC) {
            const int64_t mc = std::min(MC, m - j0);
            const size_t first = (size_t)q0 * m + j0;   // the chunk's first pair in the caller's matrices
            for (size_t p = 0; p < NP; ++p) {
                if (!planes[p].host) continue;
                const size_t w = planes[p].width;
                const char *src = static_cast<const char *>(planes[p].host) + first * w;
                for (int64_t i = 0; i < nqc; ++i) std::memcpy(hp[p] + (size_t)i * mc * w, src + (size_t)i * m * w, (size_t)mc * w);
                HAC_HIP(hipMemcpyAsync(planes[p].dev->p, hp[p], (size_t)nqc * mc * w, hipMemcpyHostToDevice, x.stream));
            }
            HAC_TRY(launch(nqc, mc));
            HAC_HIP(hipMemcpyAsync(res, out_dev.p, (size_t)nqc * mc * sizeof(Out), hipMemcpyDeviceToHost, x.stream));
            HAC_HIP(hipStreamSynchronize(x.stream));
            for (int64_t i = 0; i < nqc; ++i) {
                Out *dst = out + first + (size_t)i * m;
                const Out *r = res + (size_t)i * mc;
                if (!has_skip) {
                    std::memcpy(dst, r, (size_t)mc * sizeof(Out));
                } else {
                    const int64_t *ir = ids + first + (size_t)i * m;
                    for (int64_t j = 0; j < mc; ++j)
                        if (ir[j] != skip) dst[j] = r[j];
                }
            }
        }
    }
    return HAC_OK;
}
// D[i][j] = score(q[i], row ids[i][j]) for the pairs this shard owns: local ids, -1 = a padding slot (-FLT_MAX); 12 bytes per pair
int score_ids_host(DeviceIndex &x, const float *q, int64_t nq, const int64_t *ids, int64_t m, float *D, bool has_skip, int64_t skip) {
    const PairPlane planes[] = {{ids, 8, &x.ws_ids}};
    return pair_matrix_host(x, q, nq, m, planes, D, x.ws_D, has_skip, skip, [&](int64_t nqc, int64_t mc) {
        return score_ids_device(x, (const float *)x.ws_q.p, nqc, (const int64_t *)x.ws_ids.p, mc, (float *)x.ws_D.p, x.stream);
    });
}
// ref_score == null: rank_ids (ids: local row ids, -1 = padding); otherwise count_ahead with ids as the bounds (what a shard of a
// multi-device index is asked: the scores come from the shard that owns the row).  20 bytes per pair either way.
int rank_host(DeviceIndex &x, const float *q, int64_t nq, const int64_t *ids, const float *ref_score, int64_t m, int64_t *out) {
    const PairPlane planes[] = {{ids, 8, &x.ws_ids}, {ref_score, 4, &x.ws_D}};
    return pair_matrix_host(x, q, nq, m, planes, out, x.ws_I, false, 0, [&](int64_t nqc, int64_t mc) {
        const float *qd = (const float *)x.ws_q.p;
        const int64_t *id = (const int64_t *)x.ws_ids.p;
        if (ref_score) return count_ahead_device(x, "count_ahead", qd, nqc, (const float *)x.ws_D.p, id, false, mc, (int64_t *)x.ws_I.p, x.stream);
        return rank_ids_device(x, qd, nqc, id, mc, (int64_t *)x.ws_I.p, x.stream);
    });
}

// the host's side of the packed key (flat_ip.hip: ord2f, make_key)
float key_score_host(u64 key) {
    const u32 o = (u32)(key >> 32), b = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
    float f;
    std::memcpy(&f, &b, 4);
    return f;
}
int64_t key_row_host(u64 key) { return (int64_t)(0xFFFFFFFFu - (u32)key); }

// (D, I)[i][j] = entry_at(q[i], ranks[i][j]): the ranks are values, not ids, so nothing is checked or skipped; the pairs' keys
// come back through I's own memory (8 bytes per pair either way) and are unpacked in place.  16 bytes per pair.
int entries_at_host(DeviceIndex &x, const float *q, int64_t nq, const int64_t *ranks, int64_t m, float *D, int64_t *I) {
    const PairPlane planes[] = {{ranks, 8, &x.ws_ids}};
    u64 *keys = reinterpret_cast<u64 *>(I);
    HAC_TRY(pair_matrix_host(x, q, nq, m, planes, keys, x.ws_I, false, 0, [&](int64_t nqc, int64_t mc) {
        return entries_at_keys_device(x, "entries_at", (const float *)x.ws_q.p, nqc, (const int64_t *)x.ws_ids.p, mc, (u64 *)x.ws_I.p, 0u, x.stream);
    }));
    for (int64_t i = 0; i < nq * m; ++i) {
        u64 key;
        std::memcpy(&key, &keys[i], 8);
        D[i] = key ? key_score_host(key) : -FLT_MAX;
        I[i] = key ? key_row_host(key) : -1;
    }
    return HAC_OK;
}

// Range search over one shard's rows: lims [nq + 1] always; when the shard's total fits cap, its keys, every query's segment
// sorted, the rows in the numbering of the whole index (several devices: remap_keys, which keeps a sorted list sorted).
int remap_keys(hac_index *idx, int si, u64 *keys, int64_t n);   // (search_host.inc)
int range_host(hac_index *idx, int si, const float *q, int64_t nq, const float *radius, int64_t cap, std::vector<int64_t> &lims, std::vector<u64> &keys) {
    DeviceIndex &x = *idx->shards[si];
    DeviceGuard g(x.device);
    if (!g.ok) return fail(HAC_ERR_HIP, "cannot select HIP device %d", x.device);
    const size_t qbytes = (size_t)nq * x.d * 4, rbytes = (size_t)nq * 4, lbytes = (size_t)(nq + 1) * 8;
    HAC_TRY(x.ws_q.reserve(qbytes));
    HAC_TRY(x.ws_D.reserve(rbytes));
    char *slab = nullptr;   // queries, radii; then lims
    HAC_TRY(pin_slab(x, std::max(qbytes + rbytes, lbytes), slab));
    std::memcpy(slab, q, qbytes);
    std::memcpy(slab + qbytes, radius, rbytes);
    HAC_HIP(hipMemcpyAsync(x.ws_q.p, slab, qbytes, hipMemcpyHostToDevice, x.stream));
    HAC_HIP(hipMemcpyAsync(x.ws_D.p, slab + qbytes, rbytes, hipMemcpyHostToDevice, x.stream));
    const u64 *keys_dev = nullptr;
    HAC_TRY(range_device(x, "range_search", (const float *)x.ws_q.p, nq, (const float *)x.ws_D.p, cap, nullptr, nullptr, nullptr, nullptr, x.stream, &keys_dev));
    // (the slab's reuse is ordered behind the uploads by the stream)
    HAC_HIP(hipMemcpyAsync(slab, RangeWs(x.ws_range.p, nq, range_cap(x, nq, cap)).lims, lbytes, hipMemcpyDeviceToHost, x.stream));
    HAC_HIP(hipStreamSynchronize(x.stream));
    lims.resize((size_t)nq + 1);
    std::memcpy(lims.data(), slab, lbytes);
    const int64_t total = lims[(size_t)nq];
    keys.clear();
    if (total == 0 || total > cap) return HAC_OK;
    HAC_TRY(remap_keys(idx, si, const_cast<u64 *>(keys_dev), total));
    keys.resize((size_t)total);
    const int64_t chunk = (int64_t)8 << 20;   // 64 MiB of keys through the pinned slab at a time
    HAC_TRY(pin_slab(x, (size_t)std::min(chunk, total) * 8, slab));
    for (int64_t done = 0; done < total; done += chunk) {
        const size_t n = (size_t)std::min(chunk, total - done);
        HAC_HIP(hipMemcpyAsync(slab, keys_dev + done, n * 8, hipMemcpyDeviceToHost, x.stream));
        HAC_HIP(hipStreamSynchronize(x.stream));
        std::memcpy(keys.data() + done, slab, n * 8);
    }
    return HAC_OK;
}

// ---- the caller's ids.  The first id outside [-1, ntotal) of a host matrix [rows][cols]: the host entry points refuse it (the
// *_device ones cannot look).  `where` words its place: flat ("position %lld") or by (query, column); `pad` words what -1 is.
enum class IdPlace { FLAT, QUERY_COLUMN };
int check_host_ids(const char *what, const int64_t *ids, int64_t rows, int64_t cols, int64_t ntotal, IdPlace where, const char *pad = "a padding slot") {
    for (int64_t i = 0; i < rows * cols; ++i) {
        if (ids[i] >= -1 && ids[i] < ntotal) continue;
        char place[80];
        if (where == IdPlace::FLAT) snprintf(place, sizeof place, "position %lld", (long long)i);
        else snprintf(place, sizeof place, "(query %lld, column %lld)", (long long)(i / cols), (long long)(i % cols));
        return fail(HAC_ERR_INVALID, "%s: id %lld at %s is outside [0, %lld) (-1 = %s)", what, (long long)ids[i], place, (long long)ntotal, pad);
    }
    return HAC_OK;
}

// Global row id -> (shard, shard-local row) on an index of several devices: the inverse of remap_positions_kernel, on the host.
// Every shard's share of every add() is a span; by first global row the spans tile [0, ntotal).
struct RowLocator {
    struct Span { int64_t global0, count, local0; int shard; };
    int S;
    std::vector<Span> spans;
    std::vector<int64_t> before;   // [span][shard]: that shard's rows in the spans in front of this one
    explicit RowLocator(const hac_index *idx) : S((int)idx->shards.size()) {
        for (int s = 0; s < S; ++s)
            for (const SpanDesc &sp : idx->spans[s]) spans.push_back(Span{(int64_t)sp.global0, (int64_t)sp.count, (int64_t)sp.local0, s});
        std::sort(spans.begin(), spans.end(), [](const Span &a, const Span &b) { return a.global0 < b.global0; });
        std::vector<int64_t> rows(S, 0);
        for (const Span &sp : spans) {
            before.insert(before.end(), rows.begin(), rows.end());
            rows[sp.shard] += sp.count;
        }
    }
    // The one pass over the caller's (checked) ids: per id the span that holds it, -1 for a padding slot.
    std::vector<int32_t> locate(const int64_t *ids, size_t count) const {
        std::vector<int32_t> at(count, -1);
        const auto starts_behind = [](int64_t id, const Span &sp) { return id < sp.global0; };
        for (size_t i = 0; i < count; ++i)   // the last span with global0 <= id
            if (ids[i] >= 0) at[i] = (int32_t)(std::upper_bound(spans.begin(), spans.end(), ids[i], starts_behind) - spans.begin()) - 1;
        return at;
    }
    // of an id and its span: the shard that holds the row (a padding slot: shard 0, which writes the all-ones row / -FLT_MAX) ...
    int shard(int32_t at) const { return at < 0 ? 0 : spans[at].shard; }
    // ... its row there (-1: padding) ...
    int64_t local(int32_t at, int64_t id) const { return at < 0 ? -1 : spans[at].local0 + (id - spans[at].global0); }
    // ... and b_s(id), the number of shard s's rows with a global id below id: the row itself on its own shard (a shard's local
    // order is the global order), the rows of the spans in front on the others
    int64_t rows_below(int32_t at, int64_t id, int s) const { return at < 0 ? -1 : s == spans[at].shard ? local(at, id) : before[(size_t)at * S + s]; }
};

// several devices: every shard scores the pairs whose row it holds (padding slots: shard 0) and leaves the others' slots of D alone
int score_ids_shards(hac_index *idx, const RowLocator &loc, const std::vector<int32_t> &at, const float *q, int64_t nq, const int64_t *ids, int64_t m, float *D) {
    constexpr int64_t NOT_MINE = -2;
    std::vector<std::vector<int64_t>> local(loc.S, std::vector<int64_t>(at.size(), NOT_MINE));
    for (size_t i = 0; i < at.size(); ++i) local[loc.shard(at[i])][i] = loc.local(at[i], ids[i]);
    return for_each_shard(idx, [&](int si) { return score_ids_host(*idx->shards[si], q, nq, local[si].data(), m, D, true, NOT_MINE); });
}

// ---- removing rows (hac_index_remove_ids).  rem: this shard's removed rows, local numbering, sorted ascending, no duplicates.
// What can fail cheaply on a shard, before any shard moves a row: the staging buffers, the id list's device buffer, the slab.
constexpr int64_t REMOVE_ID_CHUNK = (int64_t)4 << 20;   // ids per upload through the pinned slab (16 MiB)
int remove_reserve(DeviceIndex &x, size_t R) {
    if (R == 0) return HAC_OK;
    DeviceGuard g(x.device);
    if (!g.ok) return fail(HAC_ERR_HIP, "cannot select HIP device %d", x.device);
    HAC_TRY(x.stage_reserve());
    HAC_TRY(x.ws_ids.reserve(R * 4));
    return x.pin_reserve((size_t)std::min<int64_t>((int64_t)R, REMOVE_ID_CHUNK) * 4);
}
// The shard's rows without rem, in place, on the shard's own stream; synchronous.
//
// Groups in front of the first removed row are not touched.  Behind it the destination rows go in ascending chunks of at most
// stage_rows() rows: compact_rows_kernel gathers a chunk into ws_stage[0] (T64 form), device-to-device copies then put the staged
// groups in their place, one copy per segment piece.  Source and destination are found through the same segment table: segments
// keep their capacities and fill order, and every segment but the last is full, so the table of the old numbering is the table of
// the new one for every row below the new total.
// Why in place is safe: src(j) >= j.  A chunk [a, b) reads old rows >= a and overwrites old rows in [a, b) only, i.e. rows below
// its own end; every earlier chunk wrote below a and every later chunk reads at or beyond b, so no chunk reads a row another has
// overwritten.  Within a chunk the stream puts every read (the gather) in front of the first write (the copies).
// Memory: ws_stage and the id list, nothing that grows with the corpus.
int remove_rows_shard(DeviceIndex &x, const std::vector<u32> &rem) {
    const int64_t R = (int64_t)rem.size();
    if (R == 0) return HAC_OK;
    DeviceGuard g(x.device);
    if (!g.ok) return fail(HAC_ERR_HIP, "cannot select HIP device %d", x.device);
    HAC_TRY(remove_reserve(x, (size_t)R));
    char *slab = nullptr;
    for (int64_t done = 0; done < R; done += REMOVE_ID_CHUNK) {
        const size_t m = (size_t)std::min(REMOVE_ID_CHUNK, R - done);
        HAC_TRY(pin_slab(x, m * 4, slab));
        std::memcpy(slab, rem.data() + done, m * 4);
        HAC_HIP(hipMemcpyAsync((u32 *)x.ws_ids.p + done, slab, m * 4, hipMemcpyHostToDevice, x.stream));
    }
    HAC_TRY(x.upload_segs(x.stream));   // (the table of the rows as they are)
    const int64_t new_rows = x.ntotal - R, first = (int64_t)rem[0];
    const int64_t g_first = first / GROUP_ROWS, g_end = (new_rows + GROUP_ROWS - 1) / GROUP_ROWS, chunk_groups = x.stage_rows() / GROUP_ROWS;
    const size_t gbytes = (size_t)GROUP_ROWS * x.d * 4;
    for (int64_t ga = g_first; ga < g_end; ga += chunk_groups) {
        const int64_t gb = std::min(ga + chunk_groups, g_end);
        compact_rows_kernel<<<dim3((unsigned)(gb - ga)), dim3(256), 0, x.stream>>>(x.d_segs, x.nseg_live, (const u32 *)x.ws_ids.p, (u32)R, (long)(ga * GROUP_ROWS),
                                                                                  (long)new_rows, x.K4, reinterpret_cast<f4 *>(x.ws_stage[0].p));
        HAC_HIP(hipGetLastError());
        int64_t gs = 0;   // the segment's first group, as upload_segs numbers it
        for (Segment &s : x.segs) {
            if (s.rows == 0) continue;
            const int64_t ng = (s.rows + GROUP_ROWS - 1) / GROUP_ROWS, lo = std::max(ga, gs), hi = std::min(gb, gs + ng);
            if (lo < hi)
                HAC_HIP(hipMemcpyAsync((char *)s.buf + (size_t)(lo - gs) * gbytes, (const char *)x.ws_stage[0].p + (size_t)(lo - ga) * gbytes, (size_t)(hi - lo) * gbytes,
                                       hipMemcpyDeviceToDevice, x.stream));
            gs += ng;
        }
    }
    // The segments' rows from the new total, in fill order.  An image that was complete is complete again when the call returns:
    // current up to the first changed group, then rebuilt from the tiles over the changed groups on the same stream; an
    // incomplete one stays incomplete (lowered), a segment without one gets none.
    int64_t r0 = 0, left = new_rows;
    for (Segment &s : x.segs) {
        const int64_t old = s.rows, changed = std::min(old, std::max<int64_t>(0, first - r0) / GROUP_ROWS * GROUP_ROWS);
        const bool h_full = s.hbuf && s.h_rows == old, r_full = s.rbuf && s.r_rows == old;
        s.rows = std::min(old, left);
        s.h_rows = std::min({s.h_rows, changed, s.rows});
        s.r_rows = std::min({s.r_rows, changed, s.rows});
        if (h_full) HAC_TRY(x.fill_half_image(s, x.stream));
        if (r_full) HAC_TRY(x.fill_row_image(s, x.stream));
        left -= s.rows;
        r0 += old;
    }
    HAC_HIP(hipStreamSynchronize(x.stream));
    // Segments left empty behind the last live one go, with their images (the first stays, as after reset()): add() then
    // continues in a partial last segment, and every segment but the last holds a multiple of 64 rows.
    while (x.segs.size() > 1 && x.segs.back().rows == 0) {
        Segment &s = x.segs.back();
        HAC_HIP(hipFree(s.buf));
        if (s.hbuf) HAC_HIP(hipFree(s.hbuf));
        if (s.rbuf) HAC_HIP(hipFree(s.rbuf));
        x.segs.pop_back();
    }
    x.ntotal = new_rows;
    x.segs_dirty = true;
    // as add() leaves them.  ws_norm (the largest |x|^2, the scale of the prefilter's certificate) stays as it is: a bound that
    // held for a superset of the rows holds for the rows that are left.
    x.half_image_unavailable = false;
    x.row_image_unavailable = false;
    x.split_searches_since_add = 0;
    x.light_searches_since_add = 0;
    return HAC_OK;
}

// The span tables of a multi-device index after the rows rem (global numbering, sorted, no duplicates) have gone.  The survivors
// of a span are still consecutive in the new global numbering and in the shard's: rows -= the removed rows inside the span,
// global0 -= the removed rows below the old global0, local0 = the running sum of the shard's spans; empty spans are dropped.
void rewrite_spans_after_remove(std::vector<std::vector<SpanDesc>> &spans, const std::vector<int64_t> &rem) {
    for (std::vector<SpanDesc> &shard : spans) {
        std::vector<SpanDesc> kept;
        u32 local0 = 0;
        for (const SpanDesc &sp : shard) {
            const int64_t below = std::lower_bound(rem.begin(), rem.end(), (int64_t)sp.global0) - rem.begin();
            const int64_t inside = (std::lower_bound(rem.begin(), rem.end(), (int64_t)sp.global0 + sp.count) - rem.begin()) - below;
            const u32 count = sp.count - (u32)inside;
            if (count == 0) continue;
            kept.push_back(SpanDesc{local0, count, sp.global0 - (u32)below, 0u});
            local0 += count;
        }
        shard.swap(kept);
    }
}
}  // namespace

extern "C" {

int hac_index_remove_ids(hac_index *idx, const int64_t *ids, int64_t n, int64_t *n_removed) {
    if (n_removed) *n_removed = 0;
    if (!idx) return fail(HAC_ERR_INVALID, "null index");
    if (n < 0 || (n > 0 && !ids)) return fail(HAC_ERR_INVALID, "remove_ids: bad arguments");
    HAC_TRY(check_host_ids("remove_ids", ids, 1, n, idx->ntotal, IdPlace::FLAT));
    std::vector<int64_t> rem;
    for (int64_t i = 0; i < n; ++i)
        if (ids[i] >= 0) rem.push_back(ids[i]);
    std::sort(rem.begin(), rem.end());
    rem.erase(std::unique(rem.begin(), rem.end()), rem.end());
    if (rem.empty()) return HAC_OK;   // nothing named: nothing is touched, the segment table stays as it is
    const int S = (int)idx->shards.size();
    std::vector<std::vector<u32>> local(S);
    if (S == 1) {
        local[0].assign(rem.begin(), rem.end());
    } else {   // a shard's local order is the global order: its list comes out sorted
        const RowLocator loc(idx);
        const std::vector<int32_t> at = loc.locate(rem.data(), rem.size());
        for (size_t i = 0; i < rem.size(); ++i) local[loc.shard(at[i])].push_back((u32)loc.local(at[i], rem[i]));
    }
    // everything that can fail cheaply on every shard first, then the kernels
    HAC_TRY(for_each_shard(idx, [&](int si) { return remove_reserve(*idx->shards[si], local[si].size()); }));
    HAC_TRY(for_each_shard(idx, [&](int si) { return remove_rows_shard(*idx->shards[si], local[si]); }));
    if (S > 1) {
        rewrite_spans_after_remove(idx->spans, rem);
        for (int si = 0; si < S; ++si) idx->spans_dirty[si] = 1;
    }
    idx->ntotal -= (int64_t)rem.size();
    if (n_removed) *n_removed = (int64_t)rem.size();
    return HAC_OK;
}

int hac_index_reconstruct_ids(hac_index *idx, const int64_t *ids, int64_t n, float *out) {
    if (!idx) return fail(HAC_ERR_INVALID, "null index");
    if (n < 0 || (n > 0 && (!ids || !out))) return fail(HAC_ERR_INVALID, "reconstruct: bad arguments");
    if (n == 0) return HAC_OK;
    HAC_TRY(check_host_ids("reconstruct", ids, 1, n, idx->ntotal, IdPlace::FLAT));
    const int S = (int)idx->shards.size();
    if (S == 1) return read_rows_host(*idx->shards[0], ids, nullptr, 0, n, out);
    const RowLocator loc(idx);
    const std::vector<int32_t> at = loc.locate(ids, (size_t)n);
    std::vector<std::vector<int64_t>> local(S), pos(S);
    for (int64_t i = 0; i < n; ++i) {
        const int sh = loc.shard(at[i]);
        local[sh].push_back(loc.local(at[i], ids[i]));
        pos[sh].push_back(i);
    }
    return for_each_shard(idx, [&](int si) { return read_rows_host(*idx->shards[si], local[si].data(), pos[si].data(), 0, (int64_t)local[si].size(), out); });
}

int hac_index_reconstruct(hac_index *idx, int64_t i0, int64_t n, float *out) {
    if (!idx) return fail(HAC_ERR_INVALID, "null index");
    if (i0 < 0 || n < 0 || i0 > idx->ntotal || n > idx->ntotal - i0)
        return fail(HAC_ERR_INVALID, "reconstruct: rows [%lld, %lld + %lld) are not inside [0, %lld]", (long long)i0, (long long)i0, (long long)n,
                    (long long)idx->ntotal);
    if (n == 0) return HAC_OK;
    if (!out) return fail(HAC_ERR_INVALID, "reconstruct: bad arguments");
    if (idx->shards.size() == 1) return read_rows_host(*idx->shards[0], nullptr, nullptr, i0, n, out);
    // several devices: consecutive rows alternate between the shards with every add(); the range goes by id, a chunk at a time
    const int64_t chunk = idx->shards[0]->stage_rows();
    std::vector<int64_t> ids((size_t)std::min(chunk, n));
    for (int64_t done = 0; done < n; done += chunk) {
        const int64_t m = std::min(chunk, n - done);
        std::iota(ids.begin(), ids.begin() + m, i0 + done);
        HAC_TRY(hac_index_reconstruct_ids(idx, ids.data(), m, out + (size_t)done * idx->d));
    }
    return HAC_OK;
}

int hac_index_reconstruct_device(hac_index *idx, const int64_t *ids_dev, int64_t i0, int64_t n, float *out_dev, void *hip_stream) {
    return on_single_shard(idx, "reconstruct_device", [&](DeviceIndex &s) -> int {
        if (n < 0 || (n > 0 && !out_dev)) return fail(HAC_ERR_INVALID, "reconstruct_device: bad arguments");
        if (ids_dev) return rows_ids_device(s, ids_dev, n, out_dev, (hipStream_t)hip_stream);
        return rows_range_device(s, i0, n, out_dev, (hipStream_t)hip_stream);
    });
}

int hac_index_score_ids(hac_index *idx, const float *q, int64_t nq, const int64_t *ids, int64_t m, float *D) {
    if (!idx) return fail(HAC_ERR_INVALID, "null index");
    if (nq < 0 || m < 0 || (nq > 0 && m > 0 && (!q || !ids || !D))) return fail(HAC_ERR_INVALID, "score_ids: bad arguments");
    if (nq == 0 || m == 0) return HAC_OK;
    HAC_TRY(check_host_ids("score_ids", ids, nq, m, idx->ntotal, IdPlace::FLAT));
    if (idx->shards.size() == 1) return score_ids_host(*idx->shards[0], q, nq, ids, m, D, false, 0);
    const RowLocator loc(idx);
    return score_ids_shards(idx, loc, loc.locate(ids, (size_t)(nq * m)), q, nq, ids, m, D);
}

int hac_index_score_ids_device(hac_index *idx, const float *q_dev, int64_t nq, const int64_t *ids_dev, int64_t m, float *D_dev, void *hip_stream) {
    return on_single_shard(idx, "score_ids_device", [&](DeviceIndex &s) -> int {
        if (nq < 0 || m < 0 || (nq > 0 && m > 0 && (!q_dev || !ids_dev || !D_dev))) return fail(HAC_ERR_INVALID, "score_ids_device: bad arguments");
        return score_ids_device(s, q_dev, nq, ids_dev, m, D_dev, (hipStream_t)hip_stream);
    });
}

int hac_index_count_ahead_device(hac_index *idx, const float *q_dev, int64_t nq, const float *ref_score_dev, const int64_t *ref_bound_dev, int64_t m,
                                 int64_t *count_dev, void *hip_stream) {
    return on_single_shard(idx, "count_ahead_device", [&](DeviceIndex &s) -> int {
        if (nq < 0 || m < 0 || (nq > 0 && m > 0 && (!q_dev || !ref_score_dev || !ref_bound_dev || !count_dev)))
            return fail(HAC_ERR_INVALID, "count_ahead_device: bad arguments");
        return count_ahead_device(s, "count_ahead_device", q_dev, nq, ref_score_dev, ref_bound_dev, false, m, count_dev, (hipStream_t)hip_stream);
    });
}

int hac_index_rank_ids_device(hac_index *idx, const float *q_dev, int64_t nq, const int64_t *ids_dev, int64_t m, int64_t *rank_dev, void *hip_stream) {
    return on_single_shard(idx, "rank_ids_device", [&](DeviceIndex &s) -> int {
        if (nq < 0 || m < 0 || (nq > 0 && m > 0 && (!q_dev || !ids_dev || !rank_dev))) return fail(HAC_ERR_INVALID, "rank_ids_device: bad arguments");
        return rank_ids_device(s, q_dev, nq, ids_dev, m, rank_dev, (hipStream_t)hip_stream);
    });
}

int hac_index_rank_ids(hac_index *idx, const float *q, int64_t nq, const int64_t *ids, int64_t m, int64_t *rank) {
    if (!idx) return fail(HAC_ERR_INVALID, "null index");
    if (nq < 0 || m < 0 || (nq > 0 && m > 0 && (!q || !ids || !rank))) return fail(HAC_ERR_INVALID, "rank_ids: bad arguments");
    if (nq == 0 || m == 0) return HAC_OK;
    HAC_TRY(check_host_ids("rank_ids", ids, nq, m, idx->ntotal, IdPlace::QUERY_COLUMN));
    const int S = (int)idx->shards.size();
    if (S == 1) return rank_host(*idx->shards[0], q, nq, ids, nullptr, m, rank);
    // Several devices.  The reference scores come from the shard that owns the row (score_ids_shards); every shard then counts
    // its own rows ahead of (score, bound), the bound translated into its numbering (RowLocator::rows_below).  A shard's local
    // order preserves the global order, so a tie still breaks by global row; the counts of the shards add up.
    const size_t total = (size_t)(nq * m);
    const RowLocator loc(idx);
    const std::vector<int32_t> at = loc.locate(ids, total);
    std::vector<float> scores(total);
    HAC_TRY(score_ids_shards(idx, loc, at, q, nq, ids, m, scores.data()));
    std::vector<std::vector<int64_t>> bounds(S, std::vector<int64_t>(total)), part(S, std::vector<int64_t>(total));
    for (int si = 0; si < S; ++si)
        for (size_t i = 0; i < total; ++i) bounds[si][i] = loc.rows_below(at[i], ids[i], si);
    HAC_TRY(for_each_shard(idx, [&](int si) { return rank_host(*idx->shards[si], q, nq, bounds[si].data(), scores.data(), m, part[si].data()); }));
    for (size_t i = 0; i < total; ++i) {
        int64_t sum = 0;
        for (int si = 0; si < S; ++si) sum = (sum < 0 || part[si][i] < 0) ? -1 : sum + part[si][i];   // (-1: padding or a NaN score, on every shard alike)
        rank[i] = sum;
    }
    return HAC_OK;
}

int hac_index_entries_at_keys_device(hac_index *idx, const float *q_dev, int64_t nq, const int64_t *ranks_dev, int64_t m, uint64_t *keys_dev, uint32_t pos_base,
                                     void *hip_stream) {
    return on_single_shard(idx, "entries_at_keys_device", [&](DeviceIndex &s) -> int {
        if (nq < 0 || m < 0 || (nq > 0 && m > 0 && (!q_dev || !ranks_dev || !keys_dev))) return fail(HAC_ERR_INVALID, "entries_at_keys_device: bad arguments");
        return entries_at_keys_device(s, "entries_at_keys_device", q_dev, nq, ranks_dev, m, (u64 *)keys_dev, pos_base, (hipStream_t)hip_stream);
    });
}

int hac_index_entries_at_device(hac_index *idx, const float *q_dev, int64_t nq, const int64_t *ranks_dev, int64_t m, float *D_dev, int64_t *I_dev,
                                const int64_t *id_map_dev, void *hip_stream) {
    return on_single_shard(idx, "entries_at_device", [&](DeviceIndex &s) -> int {
        if (nq < 0 || m < 0 || (nq > 0 && m > 0 && (!q_dev || !ranks_dev || !D_dev || !I_dev))) return fail(HAC_ERR_INVALID, "entries_at_device: bad arguments");
        return entries_at_device(s, q_dev, nq, ranks_dev, m, D_dev, I_dev, id_map_dev, (hipStream_t)hip_stream);
    });
}

int hac_index_entries_at(hac_index *idx, const float *q, int64_t nq, const int64_t *ranks, int64_t m, float *D, int64_t *I) {
    // (no multi-device form: the position digits of shards whose rows map to index rows through several spans do not line up)
    return on_single_shard(idx, "entries_at", [&](DeviceIndex &s) -> int {
        if (nq < 0 || m < 0 || (nq > 0 && m > 0 && (!q || !ranks || !D || !I))) return fail(HAC_ERR_INVALID, "entries_at: bad arguments");
        return entries_at_host(s, q, nq, ranks, m, D, I);
    });
}

int hac_index_range_search_device(hac_index *idx, const float *q_dev, int64_t nq, const float *radius_dev, int64_t cap, int64_t *lims_dev, float *D_dev,
                                  int64_t *I_dev, const int64_t *id_map_dev, void *hip_stream) {
    return on_single_shard(idx, "range_search_device", [&](DeviceIndex &s) -> int {
        if (nq < 0 || cap < 0 || (nq > 0 && (!q_dev || !radius_dev || !lims_dev)) || (cap > 0 && (!D_dev || !I_dev)))
            return fail(HAC_ERR_INVALID, "range_search_device: bad arguments");
        if (nq == 0) {
            if (lims_dev) HAC_HIP(hipMemsetAsync(lims_dev, 0, 8, (hipStream_t)hip_stream));
            return HAC_OK;
        }
        return range_device(s, "range_search_device", q_dev, nq, radius_dev, cap, lims_dev, cap > 0 ? D_dev : nullptr, I_dev, id_map_dev, (hipStream_t)hip_stream);
    });
}

int hac_index_range_search(hac_index *idx, const float *q, int64_t nq, const float *radius, int64_t cap, int64_t *lims, float *D, int64_t *I) {
    if (!idx) return fail(HAC_ERR_INVALID, "null index");
    if (nq < 0 || cap < 0 || (nq > 0 && (!q || !radius || !lims)) || (cap > 0 && (!D || !I))) return fail(HAC_ERR_INVALID, "range_search: bad arguments");
    if (nq == 0) {
        if (lims) lims[0] = 0;
        return HAC_OK;
    }
    // Every shard answers for its own rows (one host thread each), in the numbering of the whole index; a row is on one shard,
    // so the counts add up, and a query's list is the merge of the shards' sorted lists by key.  A shard whose own total
    // exceeds cap hands back no keys: the whole does not fit either.
    const int S = (int)idx->shards.size();
    std::vector<std::vector<int64_t>> part(S);
    std::vector<std::vector<u64>> keys(S);
    HAC_TRY(for_each_shard(idx, [&](int si) { return range_host(idx, si, q, nq, radius, cap, part[si], keys[si]); }));
    lims[0] = 0;
    for (int64_t i = 0; i < nq; ++i) {
        int64_t n = 0;
        for (int si = 0; si < S; ++si) n += part[si][i + 1] - part[si][i];
        lims[i + 1] = lims[i] + n;
    }
    if (lims[nq] > cap) return HAC_OK;   // an answer, not an error: D and I stay as they are
    std::vector<int64_t> at(S);
    for (int64_t i = 0; i < nq; ++i) {
        for (int si = 0; si < S; ++si) at[si] = part[si][i];
        for (int64_t o = lims[i]; o < lims[i + 1]; ++o) {
            int best = -1;
            u64 kbest = 0;
            for (int si = 0; si < S; ++si)
                if (at[si] < part[si][i + 1] && keys[si][(size_t)at[si]] > kbest) {
                    best = si;
                    kbest = keys[si][(size_t)at[si]];
                }
            ++at[best];
            D[o] = key_score_host(kbest);
            I[o] = key_row_host(kbest);
        }
    }
    return HAC_OK;
}

}  // extern "C"
