// Search behind a cursor (hac_index_search_after*): included by flat_ip.hip.
//
// after(q, s_ref, b, k) = the first k of { r in [0, n_rows) : s(q, r) not NaN, make_key(s(q, r), pos_base + r) < bound } by
// (score desc, row asc), where bound = make_key(s_ref, b) is the query's EXCLUSIVE upper key bound: one u64 per query, 0 = an
// exhausted list (no row packs to a key below it), all-ones = the start (every row does).  Two kernels: after_bounds_kernel
// turns (score, row) cursors into bounds; scan16_after_kernel (scan16_filter.inc) is scan16_kernel over every group with the
// lane's own query's bound tested in the epilogue.  A page costs one pass over the rows per query tile, at whatever depth the cursor stands.

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
