// Search behind a cursor (hac_index_search_after*): included by flat_ip.hip.
//
// after(q, s_ref, b, k) = the first k of { r in [0, n_rows) : s(q, r) not NaN, make_key(s(q, r), pos_base + r) < bound } by
// (score desc, row asc), where bound = make_key(s_ref, b) is the query's EXCLUSIVE upper key bound: one u64 per query, 0 = an
// exhausted list (no row packs to a key below it), all-ones = the start (every row does).  Two kernels: after_bounds_kernel
// turns (score, row) cursors into bounds; scan16_after_kernel is scan16_kernel over every group with the lane's own query's
// bound tested in the epilogue.  A page costs one pass over the rows per query tile, at whatever depth the cursor stands.

// bounds[i] of the cursor (score[i], row[i]); both null: every query starts from the start
//   a NaN score -> 0;  row -1 (a padding slot: the list had ended) -> 0;  row -2 (HAC_AFTER_START) -> all-ones, the score is
//   not read;  row < -2 (a mistake: the host form has refused it) -> 0;  otherwise the key of (score, row), a row at or above
//   2^32 - 1 packed as 2^32 - 1: no row of the index ties the score from behind it.
__global__ __launch_bounds__(256) void after_bounds_kernel(const float *score, const long long *row, long nq, u64 *bounds) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nq) return;
    u64 b = ~0ull;
    if (row) {
        const long long r = row[i];
        if (r != -2ll) {
            const float s = score[i];
            if (r < 0 || s != s) b = 0ull;
            else b = ((u64)f2ord(s + 0.0f) << 32) + (u64)(0xFFFFFFFFll - (r < 0xFFFFFFFFll ? r : 0xFFFFFFFFll));
        }
    }
    bounds[i] = b;
}

// The highest score a row below `bound` can have, for a float test in front of the u64 one: the score of the bound's high
// word.  Above +Inf's the word decodes to a NaN (the all-ones start bound), which a comparison would reject: +Inf stands in.
// A tie-inclusive bound (ord + 1) << 32 (a shard that holds no row at or before the cursor's) decodes to the next float above
// s_ref, so the rows tying s_ref pass.  Below -Inf's word no score lies: the NaN it decodes to rejects every row, as the
// bound does.
__device__ __forceinline__ float after_score_cap(u64 bound) {
    const u32 hi = (u32)(bound >> 32);
    return hi >= 0xFF800000u ? INFINITY : ord2f(hi);
}

// scan16_kernel with a per-query key bound.  Workgroup = (row stream blockIdx.x, tile of <= QT queries blockIdx.y); work item
// i is group i, i < a.n_items (all groups: no list).  Uses a.segs, a.nseg, a.q, a.nq, a.K4, a.k, a.C, a.QT, a.n_rows,
// a.n_items, a.thr_glob, a.partial, a.partial_cnt, a.pos_base of ScanArgs; bounds: [a.nq] of this launch, or null (the start
// for every query).
// Built from scan16_core.inc as scan16_kernel is: scan16_stage_queries, scan16_group_scores, scan16_row / rows_valid,
// scan16_compact_round and scan16_flush; the row-stream cursor and the append epilogue are its own.  What must hold here:
//   KEY TEST BEFORE APPEND  a row becomes a candidate only if make_key(s, pos_base + row) < bound, in addition to s >= th and
//       row < rows_valid: never a selection first and a filter afterwards, which could leave fewer than k eligible rows in a
//       list the selection has cut.
//   THRESHOLDS FROM ELIGIBLE ROWS ONLY  hence every key in a candidate buffer is an eligible row's, and a threshold -- the k-th
//       key of a compaction, or another workgroup's through thr_glob -- is the k-th best of SOME eligible rows of that query: a
//       proven lower bound of the answer's k-th score.  A threshold only filters rows that cannot be in the answer, so the
//       result does not depend on the row streams P, on where the launches are cut, or on the order of work.  There is no
//       seeding (a.thr_init is not read): a sample of rows gives bounds the rows behind the cursor cannot meet.
//   THE U64 COMPARISON IS THE DEFINITION  the float test s <= cap in front of it only spares the wave the epilogue of a group
//       that lies wholly ahead of every cursor of the tile; cap comes from the bound (after_score_cap), so it passes for the
//       start bound and for a tie-inclusive one, and a row it lets through is still decided by its key.
__global__ __launch_bounds__(SCAN_WAVES * 64) void scan16_after_kernel(ScanArgs a, const u64 *bounds) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int K4 = a.K4;
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
    const u32 nrounds = (a.n_items + stride - 1) / stride;
    const u32 hw = (u32)C - 64u * SCAN_WAVES;  // compaction high-water mark (>= k)

    // the lane's own query's bound, loaded once; a lane without a query (j >= QTr) gets 0: nothing lies below it
    const u64 bound = j < QTr ? (bounds ? bounds[q0 + j] : ~0ull) : 0ull;
    const float cap = after_score_cap(bound);

    u32 item = blockIdx.x * SCAN_WAVES + w;
    bool have = item < a.n_items;
    gf4ptr gp = group_ptr(a, have ? item : 0) + lane;
    f4 ring[PF];
#pragma unroll
    for (int i = 0; i < PF; ++i) ring[i] = gp[i * 64];

    for (u32 r = 0; r < nrounds; ++r) {
        const u32 g = item;
        const u32 nitem = item + stride;
        const bool have_next = nitem < a.n_items;
        f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (have) {
            const gf4ptr np = have_next ? group_ptr(a, nitem) + lane : gp;
            scan16_group_scores(acc, ring, gp, np, qb, QTr, K4);
        }

        __syncthreads();  // (A) last round's compactions are complete
        if (have) {
            const float th = thr[jc];
            bool anyp = false;
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) anyp |= (acc[rr] >= th && acc[rr] <= cap);
            if (__any(anyp)) {
                const int nvalid = rows_valid(a.n_rows, g);
                if (j < QTr) {
#pragma unroll
                    for (int rr = 0; rr < 16; ++rr) {
                        const int row = scan16_row(rr, lane);
                        const float s = acc[rr];
                        if (s >= th && row < nvalid) {   // (a NaN score fails s >= th: th is -inf or a score)
                            const u64 key = make_key(s, a.pos_base + g * GROUP_ROWS + row);
                            if (key < bound) {   // KEY TEST BEFORE APPEND
                                const u32 pos = atomicAdd(&cnt[j], 1u);
                                cand[(size_t)j * C + pos] = key;
                            }
                        }
                    }
                }
            }
        }
        __syncthreads();  // (B) all appends of this round are visible
        // THRESHOLDS FROM ELIGIBLE ROWS ONLY: the buffers hold nothing else
        scan16_compact_round(cand, cnt, thr, a.thr_glob + q0, C, a.k, hw, QTr, w, lane);
        item = nitem;
        have = have_next;
    }

    __syncthreads();
    scan16_flush(a, gridDim.x, q0, QTr, cand, cnt, C, w, lane);
}
