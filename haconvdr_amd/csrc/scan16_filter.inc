// The exact top-k kernels that filter rows by a bitmap, by a cursor, or by both: included by flat_ip.hip behind masked.inc
// (MaskArgs, mask_row, mask_groups_kernel) and after.inc (after_bounds_kernel, after_score_cap), whose heads define
// masked(q, M, k) and after(q, s_ref, b, k).  The third set is their intersection:
//
// masked_after(q, M, s_ref, b, k) = the first k of { r in [0, n_rows) : bit r of M set, s(q, r) not NaN,
// make_key(s(q, r), pos_base + r) < bound } by (score desc, row asc): search_masked's set cut by search_after's per-query
// EXCLUSIVE upper key bound (0 = an exhausted list, all-ones = the start).  mask_groups_kernel's lists and after_bounds_kernel's
// bounds are used as they are.  A page costs the tile's selected groups, at whatever depth the cursor stands.
//
// One body, scan16_filter<LIST, CURSOR>, and three __global__ functions that call it:
//   scan16_masked_kernel        <true,  false>  scan16_kernel over a tile's list of groups, the lane's own query's mask word tested
//   scan16_after_kernel         <false, true>   scan16_kernel over every group, the lane's own query's key bound tested
//   scan16_masked_after_kernel  <true,  true>   over a tile's list, both tested
// LIST and CURSOR are the only questions asked here.  scan16_kernel (vgrid, g_first / g_step, thr_init), scan16_grouped_kernel
// (its own compaction), count_ahead_kernel, range_emit_kernel and rank_hist_kernel keep bodies of their own: folding one in
// would take more flags than it removes.
//
// Workgroup = (row stream blockIdx.x, tile of <= QT queries blockIdx.y).  Work item i of the tile is, with LIST, group
// groups[tile][i], i < n_groups[tile] (m of MaskArgs; a.n_items is not read); without, group i, i < a.n_items (all groups; m is
// not read).  Uses a.segs, a.nseg, a.q, a.nq, a.K4, a.k, a.C, a.QT, a.n_rows, a.thr_glob, a.partial, a.partial_cnt, a.pos_base of
// ScanArgs.  With CURSOR, bounds: [a.nq] of this launch, or null (the start for every query); without, bounds is not read.
// Built from scan16_core.inc as scan16_kernel is: scan16_stage_queries, scan16_row / rows_valid, scan16_compact_round and
// scan16_flush; with LIST scan16_group_wait and scan16_group_mfma (the next group's mask word is loaded between them), without
// scan16_group_scores; the cursor over the work items and the append epilogue are this body's own.  What must hold here (a row
// is ELIGIBLE if it is selected by the lane's own query's mask -- LIST -- and lies behind that query's cursor -- CURSOR):
//   ELIGIBILITY BEFORE APPEND  (LIST: the bit test; CURSOR: the key test)  a row becomes a candidate only if s >= th,
//       row < rows_valid, with LIST the lane's own query's mask word has its bit, AND with CURSOR
//       make_key(s, pos_base + row) < bound: never a selection first and a filter afterwards -- by the mask, by the cursor, or
//       by one of them after the other --, which could leave fewer than k eligible rows in a list the selection has cut.  The
//       cursor row itself need not be selected and need not exist: the bound is a key, not a row.
//   THRESHOLDS FROM ELIGIBLE ROWS ONLY  (LIST and CURSOR)  hence every key in a candidate buffer is an eligible row's, and a
//       threshold -- the k-th key of a compaction, or another workgroup's through thr_glob -- is the k-th best of SOME eligible
//       rows of that query: a proven lower bound of the answer's k-th score.  A threshold only filters rows that cannot be in
//       the answer, so the result does not depend on the row streams P, on the order of the list or of work, or on where the
//       launches are cut.  There is no seeding (a.thr_init is not read): a sample of rows -- unmasked ones, or ones ahead of the
//       cursor -- gives bounds the eligible set cannot meet.
//   THE U64 COMPARISON IS THE DEFINITION  (CURSOR)  the float test s <= cap in front of it only spares the wave the epilogue of a
//       group that lies wholly ahead of every cursor of the tile; cap comes from the bound (after_score_cap), so it passes for
//       the start bound and for a tie-inclusive one, and a row it lets through is still decided by its key.
//   NO LOADS FROM DEAD LIST SLOTS  (LIST)  a list slot at or past n_groups[tile] holds whatever an earlier call left there.  No
//       address is formed from one: a tile with no group exits before its first prefetch, `have ? item : 0` reads slot 0 only
//       when it exists (n >= 1), and the next item is read only under have_next.
//   UNIFORM BARRIERS  (LIST)  nrounds comes from the tile's own count, which every wave of the workgroup reads alike (without
//       LIST it comes from a.n_items, a kernel argument).
template <bool LIST, bool CURSOR>
__device__ __forceinline__ void scan16_filter(const ScanArgs &a, const MaskArgs &m, const u64 *bounds) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int K4 = a.K4;
    u32 n_items = a.n_items;
    gu32ptr list = nullptr;
    if constexpr (LIST) {
        n_items = (u32)__builtin_amdgcn_readfirstlane((int)((gu32ptr)m.n_groups)[blockIdx.y]);
        if (n_items == 0u) return;   // workgroup-uniform, before any prefetch and any barrier: nothing is selected for this tile
        list = (gu32ptr)(m.groups + (size_t)blockIdx.y * m.G);
    }
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

    // LIST: the lane's own query's mask row; a lane without a query (j >= QTr) or without a mask reads row 0 and drops the word
    long mi = -1l;
    gu64ptr mrow = nullptr;
    if constexpr (LIST) {
        mi = j < QTr ? mask_row(m, q0 + j) : -1l;
        mrow = (gu64ptr)(m.masks + (size_t)(mi >= 0 ? mi : 0) * m.words);
    }
    // CURSOR: the lane's own query's bound, loaded once; a lane without a query gets 0: nothing lies below it
    u64 bound = ~0ull;
    float cap = INFINITY;
    if constexpr (CURSOR) {
        bound = j < QTr ? (bounds ? bounds[q0 + j] : ~0ull) : 0ull;
        cap = after_score_cap(bound);
    }

    // LIST: uniform values the epilogue and the compaction use in vector instructions only live in vector registers: a list
    // kernel has the list pointer and two group numbers more than scan16_kernel to keep in scalar ones, which are full there
    // (no spills)
    u32 pos_base = a.pos_base;
    u32 *tglob = a.thr_glob + q0;
    if constexpr (LIST) asm volatile("" : "+v"(pos_base), "+v"(tglob));

    u32 item = blockIdx.x * SCAN_WAVES + w;
    bool have = item < n_items;
    u32 g = item;   // the group of `item`: the list's entry, or the item itself
    u64 mw = 0ull;
    gf4ptr gp;
    if constexpr (LIST) {
        g = list[have ? item : 0];   // slot 0 exists: n_items >= 1
        gp = group_ptr(a, g) + lane;
    } else {
        gp = group_ptr(a, have ? item : 0) + lane;
    }
    f4 ring[PF];
#pragma unroll
    for (int i = 0; i < PF; ++i) ring[i] = gp[i * 64];
    if constexpr (LIST) mw = mrow[g];

    for (u32 r = 0; r < nrounds; ++r) {
        const u32 nitem = item + stride;
        const bool have_next = nitem < n_items;
        u32 g_next = LIST ? g : nitem;
        u64 mw_next = 0ull;
        f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (have) {
            if constexpr (LIST) {
                if (have_next) g_next = list[nitem];
            }
            const gf4ptr np = have_next ? group_ptr(a, g_next) + lane : gp;
            if constexpr (LIST) {
                scan16_group_wait();
                // the next group's mask word travels under this group's MFMAs (g_next == g without a next group: a live address)
                mw_next = mrow[g_next];
                scan16_group_mfma(acc, ring, gp, np, qb, QTr, K4);
            } else {
                scan16_group_scores(acc, ring, gp, np, qb, QTr, K4);
            }
        }

        __syncthreads();  // (A) last round's compactions are complete
        if (have) {
            const float th = thr[jc];
            const u64 sel = mi >= 0 ? mw : 0ull;   // LIST: the rows of this group the lane's own query may see
            bool anyp = false;
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) {
                if constexpr (CURSOR) anyp |= (acc[rr] >= th && acc[rr] <= cap);
                else anyp |= (acc[rr] >= th);
            }
            bool live = anyp;
            if constexpr (LIST) live = anyp && sel != 0ull;
            if (__any(live)) {
                const int nvalid = rows_valid(a.n_rows, g);
                if (j < QTr) {
#pragma unroll
                    for (int rr = 0; rr < 16; ++rr) {
                        const int row = scan16_row(rr, lane);
                        const float s = acc[rr];
                        // ELIGIBILITY BEFORE APPEND (a NaN score fails s >= th: th is -inf or a score)
                        bool ok;
                        if constexpr (LIST) ok = s >= th && row < nvalid && ((sel >> row) & 1ull);
                        else ok = s >= th && row < nvalid;
                        if (ok) {
                            if constexpr (CURSOR) {
                                const u64 key = make_key(s, pos_base + g * GROUP_ROWS + row);
                                if (key < bound) {
                                    const u32 pos = atomicAdd(&cnt[j], 1u);
                                    cand[(size_t)j * C + pos] = key;
                                }
                            } else {
                                const u32 pos = atomicAdd(&cnt[j], 1u);
                                cand[(size_t)j * C + pos] = make_key(s, pos_base + g * GROUP_ROWS + row);
                            }
                        }
                    }
                }
            }
        }
        __syncthreads();  // (B) all appends of this round are visible
        // THRESHOLDS FROM ELIGIBLE ROWS ONLY: the buffers hold nothing else
        scan16_compact_round(cand, cnt, thr, tglob, C, a.k, hw, QTr, w, lane);
        item = nitem;
        have = have_next;
        g = g_next;
        mw = mw_next;
    }

    __syncthreads();
    scan16_flush(a, gridDim.x, q0, QTr, cand, cnt, C, w, lane);
}

__global__ __launch_bounds__(SCAN_WAVES * 64) void scan16_masked_kernel(ScanArgs a, MaskArgs m) { scan16_filter<true, false>(a, m, nullptr); }
__global__ __launch_bounds__(SCAN_WAVES * 64) void scan16_after_kernel(ScanArgs a, const u64 *bounds) { scan16_filter<false, true>(a, MaskArgs{}, bounds); }
__global__ __launch_bounds__(SCAN_WAVES * 64) void scan16_masked_after_kernel(ScanArgs a, MaskArgs m, const u64 *bounds) { scan16_filter<true, true>(a, m, bounds); }
