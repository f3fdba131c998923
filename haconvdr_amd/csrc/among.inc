// Search among named rows (hac_index_search_among*): included by flat_ip.hip.
//
// among(q, c, k) = the first k of { rows r in set(c), 0 <= r < n_rows, s(q, r) not NaN } by key (score desc, row asc).  Two stages,
// so that one query with 4096 candidates still fills the chip:
//   among_keys_kernel     score_ids_kernel's grid and gather; where that one stores the score, this one stores the packed key
//                         of (score, pos_base + row) into a [nq][P] workspace, P = the power of two >= m; 0 for an id outside
//                         the rows, for a NaN score and for the slots m..P
//   among_select_kernel   one workgroup per query: the P keys into LDS, bitonic sort (descending), repeats dropped -- equal
//                         non-zero keys are the same row, and sorted they are neighbours --, the first k distinct non-zero keys
//                         compacted by a block prefix count into [nq][k], the rest 0
// No atomics, no threshold, no retry: the output is a pure function of the inputs, and nothing goes to the status ring.
constexpr int AMONG_THREADS = 256;
// dynamic LDS of among_select_kernel: the keys, then the wave counts of the prefix (two sets, one barrier per chunk)
constexpr size_t among_lds(u32 P) { return (size_t)P * 8 + 2 * (AMONG_THREADS / 64) * 4; }

// Workgroup = (query i, 256 consecutive slots j), the query row in LDS, one thread per slot, eight pieces in flight.  The last
// workgroup of a query also zeroes the slots behind its own 256 up to P.
// The chain loop is a third copy of rescore_kernel's (scan_split.inc), after score_ids_kernel's: that kernel's register
// allocation is pinned (see score_ids_kernel), and score_ids_kernel's own resource line stays what it is.
__global__ __launch_bounds__(256) void among_keys_kernel(const SegDesc *__restrict__ segs, const float4 *const *__restrict__ rimg_tab, int nseg,
                                                         const float *__restrict__ q, const long long *__restrict__ cand, long m,
                                                         u32 blocks_per_q, u32 P, long n_rows, int K4, u32 pos_base,
                                                         u64 *__restrict__ keys) {
    __shared__ float qs[HAC_MAX_D];
    const int tid = threadIdx.x;
    const size_t qi = blockIdx.x / blocks_per_q;
    const u32 bq = blockIdx.x % blocks_per_q;
    const long j = (long)bq * 256 + tid;
    const int d = K4 * 4;
    u64 *out = keys + qi * P;
    for (int i = tid; i < d; i += 256) qs[i] = q[qi * d + i];
    if (bq == blocks_per_q - 1)
        for (u32 t = blocks_per_q * 256 + tid; t < P; t += 256) out[t] = 0ull;
    __syncthreads();
    if (j >= (long)P) return;
    const long long id = j < m ? cand[qi * m + j] : -1ll;
    u64 key = 0ull;
    if (id >= 0 && id < n_rows) {
        size_t stride;
        const gf4ptr gp = row_pieces(segs, rimg_tab, nseg, id, K4, stride);
        float s = 0.f;
        f4 v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = gp[(size_t)i * stride];
        for (int t = 0; t < K4; t += 8) {   // (d % 32 == 0: K4 is a multiple of 8)
            f4 c[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) c[i] = v[i];
            if (t + 8 < K4) {
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = gp[(size_t)(t + 8 + i) * stride];
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                s = fmaf(c[i].x, qs[4 * (t + i) + 0], s);
                s = fmaf(c[i].y, qs[4 * (t + i) + 1], s);
                s = fmaf(c[i].z, qs[4 * (t + i) + 2], s);
                s = fmaf(c[i].w, qs[4 * (t + i) + 3], s);
            }
        }
        if (s == s) key = make_key(s, pos_base + (u32)id);   // (a NaN score is in no list; every other score packs to a non-zero key)
    }
    out[j] = key;
}

// One workgroup per query.  keys [nq][P] -> out [nq][k].  The sort is block_sort_desc (what merge_keys_kernel and
// range_sort_kernel sort with).  Reading slot i and its left neighbour is a ds_read_b64 of consecutive lanes at consecutive
// 8 bytes: no bank conflict; the sort's strides below 32 keys pay the 2-way conflict they pay in the range sort.
// The compaction walks the sorted keys in chunks of 256: ballot and popcount inside a wave, the four wave counts through LDS.
// It stops at the first chunk behind k kept keys, or at the end of the keys.
__global__ __launch_bounds__(AMONG_THREADS) void among_select_kernel(const u64 *__restrict__ keys, u32 P, int k, u64 *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u64 *buf = reinterpret_cast<u64 *>(smem);                    // [P]
    u32 *wcnt = reinterpret_cast<u32 *>(buf + P);                // [2][AMONG_THREADS / 64]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const size_t q = blockIdx.x;
    const u64 *src = keys + q * P;
    u64 *dst = out + q * (size_t)k;
    for (u32 i = tid; i < P; i += AMONG_THREADS) buf[i] = src[i];
    __syncthreads();
    if (P > 1) block_sort_desc(buf, P, tid, AMONG_THREADS);
    const u64 below = (1ull << lane) - 1ull;   // the lanes before this one
    u32 kept = 0;                              // distinct keys in front of the chunk (uniform)
    int flip = 0;
    for (u32 base = 0; base < P && kept < (u32)k; base += AMONG_THREADS, flip ^= 1) {
        const u32 i = base + tid;
        const u64 key = i < P ? buf[i] : 0ull;
        const bool first = key != 0ull && (i == 0 || buf[i - 1] != key);
        const u64 vote = __ballot(first);
        u32 *wc = wcnt + flip * (AMONG_THREADS / 64);
        if (lane == 0) wc[w] = (u32)__popcll(vote);
        __syncthreads();
        u32 at = kept + (u32)__popcll(vote & below), total = 0;
#pragma unroll
        for (int v = 0; v < AMONG_THREADS / 64; ++v) {
            const u32 c = wc[v];
            if (v < w) at += c;
            total += c;
        }
        if (first && at < (u32)k) dst[at] = key;
        kept += total;
    }
    for (u32 i = min(kept, (u32)k) + tid; i < (u32)k; i += AMONG_THREADS) dst[i] = 0ull;
}
