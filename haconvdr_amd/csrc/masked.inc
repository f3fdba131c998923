// Search inside a bitmap (hac_index_search_masked*): included by flat_ip.hip.
//
// masked(q, M, k) = the first k of { r in [0, n_rows) : bit r of M set, s(q, r) not NaN } by (score desc, row asc).  A mask is
// u64 [words], words = ceil(n_rows / 64): row r is bit r & 63 of word r >> 6, so a word is exactly one T64 group.  Two kernels:
// mask_groups_kernel lists, per query tile, the groups in which any of the tile's masks selects a row; scan16_masked_kernel
// (scan16_filter.inc) is scan16_kernel over that list, with the lane's own query's mask word tested in the epilogue.  A
// selective mask then costs its own groups and not the corpus.
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
