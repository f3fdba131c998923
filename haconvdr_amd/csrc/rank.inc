// Exact corpus rank of named rows (hac_index_rank_ids*, hac_index_count_ahead_device): included by flat_ip.hip.
//
// count_ahead(q, s_ref, b) = #{ rows r in [0, n_rows) : s(q, r) is not NaN and make_key(s(q, r), r) > make_key(s_ref, b) }
// -- the rows an unbounded search of q returns in front of the pair (s_ref, b).  One pass over the corpus in the shape of
// scan16_kernel: the same T64 row stream, the same bit-exact fp32 MFMA chain, an epilogue that COUNTS where scan16's collects.
// No candidate buffers, no thresholds, no selection: nothing here can overflow, so there is no pass bound and nothing for
// the status ring, and the waves of a workgroup never wait for each other inside the row loop.
//
// Cost: the corpus is streamed once per (tile of 16 queries, chunk of MT references); typical m is 1..4 = one chunk.
struct RankArgs {
    const float *ref_score;       // [nq][m] reference scores
    const long long *ref_bound;   // [nq][m] reference bounds: rows r < bound win a score tie
    u64 *counts;                  // [nq][m], zeroed before the launch
    long m;
    u32 chunk0;                   // blockIdx.z + chunk0 = the chunk of MT references this workgroup counts for
};

constexpr int RANK_MT = 8;
// dynamic LDS: queries [K4][QT] f4, reference keys u64 [16][MT], smallest reference score float [16], wave sums u32 [SCAN_WAVES][16][MT]
constexpr size_t rank_lds(int K4, int QT, int MT) { return (size_t)K4 * QT * 16 + (size_t)16 * MT * 8 + 64 + (size_t)SCAN_WAVES * 16 * MT * 4; }

// Workgroup = (row stream blockIdx.x, tile of <= 16 queries blockIdx.y, chunk of MT references blockIdx.z).  Uses a.segs, a.nseg,
// a.q, a.nq, a.K4, a.QT, a.n_rows, a.n_items (groups, from group 0) of ScanArgs.
// Built from scan16_core.inc: scan16_stage_queries, scan16_group_scores, scan16_row / rows_valid; the row-stream cursor is
// written out here, and the waves of a workgroup meet at no barrier inside it.
template <int MT>
__global__ __launch_bounds__(SCAN_WAVES * 64) void count_ahead_kernel(ScanArgs a, RankArgs ra) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int K4 = a.K4;
    const int q0 = blockIdx.y * a.QT;
    const int QTr = min(a.QT, a.nq - q0);
    const long col0 = ((long)blockIdx.z + ra.chunk0) * MT;

    f4 *ldsQ = reinterpret_cast<f4 *>(smem);                                        // [K4][QTr]
    u64 *refkey = reinterpret_cast<u64 *>(smem + (size_t)K4 * a.QT * 16);           // [16][MT]
    float *minref = reinterpret_cast<float *>(refkey + 16 * MT);                    // [16]
    u32 *red = reinterpret_cast<u32 *>(minref + 16);                                // [SCAN_WAVES][16][MT]

    scan16_stage_queries(ldsQ, a.q, K4, QTr, tid, [q0](int j) { return q0 + j; });
    // the references of this chunk as keys; one that can never be behind a row (NaN score, negative bound, a slot past m or
    // past the tile) is the all-ones key, which no row's key exceeds
    if (tid < 16) {
        float mn = INFINITY;
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            u64 key = ~0ull;
            if (tid < QTr && col0 + t < ra.m) {
                const size_t at = (size_t)(q0 + tid) * ra.m + col0 + t;
                const float s = ra.ref_score[at];
                const long long b = ra.ref_bound[at];
                if (s == s && b >= 0) {
                    key = make_key(s, (u32)min(b, (long long)a.n_rows));
                    mn = fminf(mn, s);
                }
            }
            refkey[tid * MT + t] = key;
        }
        minref[tid] = mn;
    }
    __syncthreads();

    const int j = lane & 15;
    const int jc = min(j, QTr - 1);
    const f4 *qb = ldsQ + jc;
    const u32 stride = gridDim.x * SCAN_WAVES;
    const u32 nrounds = (a.n_items + stride - 1) / stride;
    const float mref = minref[jc];

    u32 item = blockIdx.x * SCAN_WAVES + w;
    bool have = item < a.n_items;
    gf4ptr gp = group_ptr(a, have ? item : 0) + lane;
    f4 ring[PF];
#pragma unroll
    for (int i = 0; i < PF; ++i) ring[i] = gp[i * 64];
    u32 cnt[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) cnt[t] = 0u;

    for (u32 r = 0; r < nrounds; ++r) {
        const u32 g = item;
        const u32 nitem = item + stride;
        const bool have_next = nitem < a.n_items;
        f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (have) {
            const gf4ptr np = have_next ? group_ptr(a, nitem) + lane : gp;
            scan16_group_scores(acc, ring, gp, np, qb, QTr, K4);

            // a group none of whose scores reaches the chunk's smallest reference score counts for nothing: the common case
            // (a NaN score compares false; rows past n_rows that pass are masked below)
            bool anyp = false;
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) anyp |= (acc[rr] >= mref);
            if (__any(anyp)) {
                const int nvalid = rows_valid(a.n_rows, g);
                u64 rk[MT];
#pragma unroll
                for (int t = 0; t < MT; ++t) rk[t] = refkey[jc * MT + t];
#pragma unroll
                for (int rr = 0; rr < 16; ++rr) {
                    const int row = scan16_row(rr, lane);
                    const float s = acc[rr];
                    // f2ord of a positive NaN sorts above every score: a NaN row gets the key nothing is behind
                    const u64 key = (s == s && row < nvalid) ? make_key(s, g * GROUP_ROWS + row) : 0ull;
#pragma unroll
                    for (int t = 0; t < MT; ++t) cnt[t] += key > rk[t] ? 1u : 0u;
                }
            }
        }
        item = nitem;
        have = have_next;
    }

    // the four lane groups of a wave that share a query, then the waves, then one integer atomic per (query, reference):
    // integer sums do not depend on their order, the result is a pure function of the inputs
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        u32 c = cnt[t];
        c += (u32)__shfl_xor((int)c, 16);
        c += (u32)__shfl_xor((int)c, 32);
        if (lane < 16) red[(w * 16 + lane) * MT + t] = c;
    }
    __syncthreads();
    if (tid < 16 * MT) {
        const int jq = tid / MT, t = tid - jq * MT;
        u64 sum = 0;
#pragma unroll
        for (int ww = 0; ww < SCAN_WAVES; ++ww) sum += red[(ww * 16 + jq) * MT + t];
        if (jq < QTr && col0 + t < ra.m && sum != 0ull) atomicAdd(&ra.counts[(size_t)(q0 + jq) * ra.m + col0 + t], sum);
    }
}

// counters -> ranks, with the -1 rules: a NaN reference score, a negative bound, and (rank_ids: ids == the bounds) an id
// outside [0, n_rows)
__global__ __launch_bounds__(256) void rank_finish_kernel(const u64 *__restrict__ counts, const float *__restrict__ ref_score,
                                                          const long long *__restrict__ ref_bound, bool bounds_are_ids, long n, long n_rows,
                                                          long long *__restrict__ out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float s = ref_score[i];
    const long long b = ref_bound[i];
    const bool none = s != s || b < 0 || (bounds_are_ids && b >= n_rows);
    out[i] = none ? -1ll : (long long)counts[i];
}
