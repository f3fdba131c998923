// Search inside a bitmap (hac_index_search_masked*): included by flat_ip.hip.
//
// masked(q, M, k) = the first k of { r in [0, n_rows) : bit r of M set, s(q, r) not NaN } by (score desc, row asc).  A mask is
// u64 [words], words = ceil(n_rows / 64): row r is bit r & 63 of word r >> 6, so a word is exactly one T64 group.  Two kernels:
// mask_groups_kernel lists, per query tile, the groups in which any of the tile's masks selects a row; scan16_masked_kernel is
// scan16_kernel over that list, with the lane's own query's mask word tested in the epilogue.  A selective mask then costs its
// own groups and not the corpus.
struct MaskArgs {
    const u64 *masks;           // [n_masks][words]
    const long long *mask_of;   // [nq] the mask of each query, or null (per_query says which)
    long n_masks, words;
    int per_query;              // null mask_of: 1 = query i uses mask i (n_masks == nq), 0 = every query uses mask 0
    u32 *groups;                // [tiles][G] the tile's selected groups, in no particular order
    u32 *n_groups;              // [tiles] entries of each list (zeroed before mask_groups_kernel)
    u32 G;
};
typedef const __attribute__((address_space(1))) u64 *gu64ptr;
typedef const __attribute__((address_space(1))) u32 *gu32ptr;

// the mask row of query q (of this launch), or -1: a mask_of entry outside [0, n_masks) selects nothing (the device forms'
// rule; the host form has refused it)
__device__ __forceinline__ long mask_row(const MaskArgs &m, int q) {
    if (m.mask_of) {
        const long long v = m.mask_of[q];
        return (v >= 0 && v < m.n_masks) ? (long)v : -1l;
    }
    return m.per_query ? (long)q : 0l;
}

// Workgroup = (256 groups blockIdx.x, query tile blockIdx.y).  A thread ORs the words of its group over the tile's queries
// (consecutive threads read consecutive words), clips the last group to n_rows -- bits at or above n_rows select nothing, so a
// group whose only set bits lie there is not listed -- and the wave appends its selected groups as one dense run: ballot +
// prefix, one atomic per wave, as range_emit_kernel appends its pairs.  The order of a list therefore varies from run to run;
// nothing downstream depends on it (scan16_masked_kernel's results are a pure function of the SET of groups).
__global__ __launch_bounds__(256) void mask_groups_kernel(MaskArgs m, int nq, int QT, long n_rows) {
    const int lane = threadIdx.x & 63;
    const u32 g = blockIdx.x * 256u + threadIdx.x;
    const int q0 = blockIdx.y * QT;
    const int QTr = min(QT, nq - q0);
    u64 any = 0ull;
    if (g < m.G) {
        for (int j = 0; j < QTr; ++j) {
            const long mi = mask_row(m, q0 + j);
            if (mi >= 0) any |= m.masks[(size_t)mi * m.words + g];
        }
        const long rem = n_rows - (long)g * GROUP_ROWS;
        if (rem < GROUP_ROWS) any &= (1ull << rem) - 1ull;   // (g < G: 1 <= rem)
    }
    const bool sel = any != 0ull;
    const u64 vote = __ballot(sel);
    if (vote == 0ull) return;   // wave-uniform
    u32 start = 0;
    if (lane == 0) start = atomicAdd(&m.n_groups[blockIdx.y], (u32)__popcll(vote));
    start = (u32)__builtin_amdgcn_readfirstlane((int)start);
    // at most G groups are selected per tile: start + prefix < G
    if (sel) m.groups[(size_t)blockIdx.y * m.G + start + (u32)__popcll(vote & ((1ull << lane) - 1ull))] = g;
}

// scan16_kernel over a tile's list of groups.  Workgroup = (row stream blockIdx.x, tile of <= QT queries blockIdx.y); work item i
// of the tile is group groups[tile][i], i < n_groups[tile].  Uses a.segs, a.nseg, a.q, a.nq, a.K4, a.k, a.C, a.QT, a.n_rows,
// a.thr_glob, a.partial, a.partial_cnt, a.pos_base of ScanArgs (a.thr_init is not read: there is no seeding, a sample of
// unmasked rows would give bounds the masked set cannot meet).
// Built from scan16_core.inc as scan16_kernel is: scan16_stage_queries, scan16_group_wait and scan16_group_mfma (the next group's mask
// word is loaded between them), scan16_row / rows_valid, scan16_compact_round and scan16_flush; the cursor over the list and the
// append epilogue are its own.  What must hold here:
//   BIT TEST BEFORE APPEND  a row becomes a candidate only if the lane's own query's mask word has its bit: never a selection
//       first and a filter afterwards, which could leave fewer than k selected rows in a list the selection has cut.
//   THRESHOLDS FROM SELECTED ROWS ONLY  hence every key in a candidate buffer is a selected row's, and a threshold -- the k-th key
//       of a compaction, or another workgroup's through thr_glob -- is the k-th best of SOME selected rows of that query: a
//       proven lower bound of its masked k-th score.  A threshold only filters rows that cannot be in the answer, so the result
//       does not depend on the row streams P, on the order of the list, or on where the launches are cut.
//   NO LOADS FROM DEAD LIST SLOTS  a list slot at or past n_groups[tile] holds whatever an earlier call left there.  No address
//       is formed from one: a tile with no group exits before its first prefetch, `have ? item : 0` reads slot 0 only when it
//       exists (n >= 1), and the next item is read only under have_next.
//   UNIFORM BARRIERS  nrounds comes from the tile's own count, which every wave of the workgroup reads alike.
__global__ __launch_bounds__(SCAN_WAVES * 64) void scan16_masked_kernel(ScanArgs a, MaskArgs m) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int K4 = a.K4;
    const u32 n_items = (u32)__builtin_amdgcn_readfirstlane((int)((gu32ptr)m.n_groups)[blockIdx.y]);
    if (n_items == 0u) return;   // workgroup-uniform, before any prefetch and any barrier: nothing is selected for this tile
    gu32ptr list = (gu32ptr)(m.groups + (size_t)blockIdx.y * m.G);
    const int q0 = blockIdx.y * a.QT;
    const int QTr = min(a.QT, a.nq - q0);
    const int C = a.C;

    f4 *ldsQ = reinterpret_cast<f4 *>(smem);                       // [K4][QTr]
    u64 *cand = reinterpret_cast<u64 *>(smem + (size_t)K4 * QTr * 16);     // [QTr][C]
    u32 *cnt = reinterpret_cast<u32 *>(cand + (size_t)QTr * C);            // [16]
    float *thr = reinterpret_cast<float *>(cnt + 16);                      // [16]

    scan16_stage_queries(ldsQ, a.q, K4, QTr, tid, [q0](int j) { return q0 + j; });
    if (tid < 16) {
        cnt[tid] = 0;
        thr[tid] = -INFINITY;
    }
    __syncthreads();

    const int j = lane & 15;
    const int jc = min(j, QTr - 1);
    const f4 *qb = ldsQ + jc;
    const u32 stride = gridDim.x * SCAN_WAVES;
    const u32 nrounds = (n_items + stride - 1) / stride;
    const u32 hw = (u32)C - 64u * SCAN_WAVES;  // compaction high-water mark (>= k)

    // the lane's own query's mask row; a lane without a query (j >= QTr) or without a mask reads row 0 and drops the word
    const long mi = j < QTr ? mask_row(m, q0 + j) : -1l;
    gu64ptr mrow = (gu64ptr)(m.masks + (size_t)(mi >= 0 ? mi : 0) * m.words);

    // Uniform values the epilogue and the compaction use in vector instructions only live in vector registers: this kernel has the
    // list pointer and two group numbers more than scan16_kernel to keep in scalar ones, which are full there (no spills)
    u32 pos_base = a.pos_base;
    u32 *tglob = a.thr_glob + q0;
    asm volatile("" : "+v"(pos_base), "+v"(tglob));

    u32 item = blockIdx.x * SCAN_WAVES + w;
    bool have = item < n_items;
    u32 g = list[have ? item : 0];   // slot 0 exists: n_items >= 1
    gf4ptr gp = group_ptr(a, g) + lane;
    f4 ring[PF];
#pragma unroll
    for (int i = 0; i < PF; ++i) ring[i] = gp[i * 64];
    u64 mw = mrow[g];

    for (u32 r = 0; r < nrounds; ++r) {
        const u32 nitem = item + stride;
        const bool have_next = nitem < n_items;
        u32 g_next = g;
        u64 mw_next = 0ull;
        f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (have) {
            if (have_next) g_next = list[nitem];
            const gf4ptr np = have_next ? group_ptr(a, g_next) + lane : gp;
            scan16_group_wait();
            // the next group's mask word travels under this group's MFMAs (g_next == g without a next group: a live address)
            mw_next = mrow[g_next];
            scan16_group_mfma(acc, ring, gp, np, qb, QTr, K4);
        }

        __syncthreads();  // (A) last round's compactions are complete
        if (have) {
            const float th = thr[jc];
            const u64 sel = mi >= 0 ? mw : 0ull;   // the rows of this group the lane's own query may see
            bool anyp = false;
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) anyp |= (acc[rr] >= th);
            if (__any(anyp && sel != 0ull)) {
                const int nvalid = rows_valid(a.n_rows, g);
                if (j < QTr) {
#pragma unroll
                    for (int rr = 0; rr < 16; ++rr) {
                        const int row = scan16_row(rr, lane);
                        const float s = acc[rr];
                        // BIT TEST BEFORE APPEND (a NaN score fails s >= th: th is -inf or a score)
                        if (s >= th && row < nvalid && ((sel >> row) & 1ull)) {
                            const u32 pos = atomicAdd(&cnt[j], 1u);
                            cand[(size_t)j * C + pos] = make_key(s, pos_base + g * GROUP_ROWS + row);
                        }
                    }
                }
            }
        }
        __syncthreads();  // (B) all appends of this round are visible
        // THRESHOLDS FROM SELECTED ROWS ONLY: the buffers hold nothing else
        scan16_compact_round(cand, cnt, thr, tglob, C, a.k, hw, QTr, w, lane);
        item = nitem;
        have = have_next;
        g = g_next;
        mw = mw_next;
    }

    __syncthreads();
    scan16_flush(a, gridDim.x, q0, QTr, cand, cnt, C, w, lane);
}
