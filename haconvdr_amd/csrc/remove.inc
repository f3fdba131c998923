// Removing rows in place (hac_index_remove_ids): the compaction kernel.  Included by flat_ip.hip; the driver and the host's
// bookkeeping are in rows_host.inc ("removing rows").
//
// The survivors keep their order and are renumbered densely, so destination row j of a shard reads source row
//   src(j) = j + t,  t = the smallest index in [0, R] with rem[t] - t > j  (t = R when there is none)
// over the shard's removed rows rem[0 .. R), sorted ascending and free of duplicates: rem[t] - t is the number of survivors in
// front of rem[t], it never decreases with t, and the t it selects is the number of removed rows in front of the j-th survivor.
// One binary search per lane.
//
// One workgroup per destination group of 64 rows, lane l = row 64 g + l, wave w the chunks w, w + 4, ...: per chunk a lane reads
// its 16-byte piece at (group src / 64, lane src % 64) of the segment table -- src is monotone in j, so a wave reads a shifted
// window over the source groups -- and the wave writes one whole 1-KiB T64 chunk of the staging buffer (group blockIdx.x of the
// buffer = destination group j0 / 64 + blockIdx.x; the driver copies the staged groups to their place).  Lanes behind the last
// surviving row write zeros, for new_segment's reason: the padding rows of the last live group stay finite.  Bits only move:
// nothing here does arithmetic on a row's words, so NaN payloads, -0.0 and denormals survive.  No atomics, no scratch.
__global__ __launch_bounds__(256) void compact_rows_kernel(const SegDesc *__restrict__ segs, int nseg, const u32 *__restrict__ rem, u32 R, long j0,
                                                           long new_rows, int K4, f4 *__restrict__ stage) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long j = j0 + (long)blockIdx.x * GROUP_ROWS + lane;
    f4 *dst = stage + (size_t)blockIdx.x * K4 * GROUP_ROWS + lane;
    const bool live = j < new_rows;
    gf4ptr src = nullptr;
    if (live) {
        u32 lo = 0, hi = R;
        while (lo < hi) {
            const u32 mid = lo + ((hi - lo) >> 1);
            if ((long)rem[mid] - (long)mid > j) hi = mid;
            else lo = mid + 1;
        }
        const long s = j + (long)lo;   // < the shard's rows before the call: the j-th survivor exists for every j < new_rows
        const u32 grp = (u32)(s / GROUP_ROWS);
        const int sg = seg_of_group(segs, nseg, grp);
        src = as_global(segs[sg].ptr) + (size_t)(grp - segs[sg].gstart) * K4 * GROUP_ROWS + (u32)(s % GROUP_ROWS);
    }
    if (!live) {
        for (int c = w; c < K4; c += 4) dst[(size_t)c * GROUP_ROWS] = f4{0.f, 0.f, 0.f, 0.f};
        return;
    }
    // eight pieces in flight per lane while the wave has that many chunks left
    int c = w;
    for (; c + 28 < K4; c += 32) {
        f4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = src[(size_t)(c + 4 * u) * GROUP_ROWS];
#pragma unroll
        for (int u = 0; u < 8; ++u) dst[(size_t)(c + 4 * u) * GROUP_ROWS] = v[u];
    }
    for (; c < K4; c += 4) dst[(size_t)c * GROUP_ROWS] = src[(size_t)c * GROUP_ROWS];
}
