// Range search (hac_index_range_search*): included by flat_ip.hip.
//
// range(q, r) = { rows x in [0, n_rows) : s(q, x) is not NaN and s(q, x) > r }, ordered by key (score desc, row asc): the head
// of an unbounded search of q, as long as the scores say.  count_ahead_kernel's pass with an epilogue that EMITS where that
// one counts:
//   range_emit_kernel     one pass over the rows per tile of 16 queries: per-query counters (always exact) and (query, key)
//                         pairs appended to a staging buffer through one cursor; pairs at or behind `cap` are dropped
//   range_offsets_kernel  lims = exclusive scan of the counters; the fits / overflows word every later kernel reads first
//   range_scatter_kernel  staged pairs -> their query's segment [lims[i], lims[i + 1])
//   range_sort_kernel     blocks of RANGE_SORT_N keys of a segment, bitonic in LDS
//   range_merge_kernel    one pass of pairwise merges of sorted runs between two buffers (merge path, a tile of
//                         RANGE_SORT_N outputs per workgroup)
//   range_results_kernel  keys -> (D, I) in [0, lims[nq]), id_map applied
// The order atomics resolve in decides where a pair is staged and scattered to, never what the sorted segment holds: keys are
// unique (the row is in the key), so the result is a pure function of the inputs.  Nothing here selects, thresholds or retries:
// no pass bound, nothing for the status ring, and no kernel waits for another workgroup.
struct RangeArgs {
    const float *radius;   // [nq] of the launch's queries
    u64 *counts;           // [nq] of the launch's queries, zeroed before the first launch
    u64 *cursor;           // pairs emitted so far by all launches (ctl[RANGE_CURSOR])
    u64 *stage_key;        // [cap]
    u32 *stage_q;          // [cap] query of the pair, numbered over the whole call
    u64 cap;
    u32 q_base;            // the launch's first query in the whole call
};

constexpr int RANGE_SORT_N = 4096;   // keys one workgroup sorts in LDS (32 KiB), and the outputs of one merge tile
constexpr int RANGE_THREADS = 256;
// control words (u64) in front of the workspace
constexpr int RANGE_CURSOR = 0, RANGE_TOTAL = 1, RANGE_FITS = 2, RANGE_CTL_WORDS = 4;
// dynamic LDS of range_emit_kernel: queries [K4][QT] f4, radius float [16], wave sums u32 [SCAN_WAVES][16]
constexpr size_t range_lds(int K4, int QT) { return (size_t)K4 * QT * 16 + 64 + (size_t)SCAN_WAVES * 16 * 4; }

// Workgroup = (row stream blockIdx.x, tile of <= 16 queries blockIdx.y).  Uses a.segs, a.nseg, a.q, a.nq, a.K4, a.QT, a.n_rows,
// a.n_items (groups, from group 0) of ScanArgs.  Built from scan16_core.inc as count_ahead_kernel is: scan16_stage_queries,
// scan16_group_scores, scan16_row / rows_valid; the row-stream cursor is written out here.
__global__ __launch_bounds__(SCAN_WAVES * 64) void range_emit_kernel(ScanArgs a, RangeArgs ra) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int K4 = a.K4;
    const int q0 = blockIdx.y * a.QT;
    const int QTr = min(a.QT, a.nq - q0);

    f4 *ldsQ = reinterpret_cast<f4 *>(smem);                                        // [K4][QTr]
    float *rad_lds = reinterpret_cast<float *>(smem + (size_t)K4 * a.QT * 16);      // [16]
    u32 *red = reinterpret_cast<u32 *>(rad_lds + 16);                               // [SCAN_WAVES][16]

    scan16_stage_queries(ldsQ, a.q, K4, QTr, tid, [q0](int j) { return q0 + j; });
    // a slot past the tile gets the radius no score exceeds (so does a NaN radius, by the compare itself)
    if (tid < 16) rad_lds[tid] = tid < QTr ? ra.radius[q0 + tid] : INFINITY;
    __syncthreads();

    const int j = lane & 15;
    const int jc = min(j, QTr - 1);
    const f4 *qb = ldsQ + jc;
    const u32 stride = gridDim.x * SCAN_WAVES;
    const u32 nrounds = (a.n_items + stride - 1) / stride;
    const float rad = rad_lds[j];

    u32 item = blockIdx.x * SCAN_WAVES + w;
    bool have = item < a.n_items;
    gf4ptr gp = group_ptr(a, have ? item : 0) + lane;
    f4 ring[PF];
#pragma unroll
    for (int i = 0; i < PF; ++i) ring[i] = gp[i * 64];
    u32 cnt = 0u;

    for (u32 r = 0; r < nrounds; ++r) {
        const u32 g = item;
        const u32 nitem = item + stride;
        const bool have_next = nitem < a.n_items;
        f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (have) {
            const gf4ptr np = have_next ? group_ptr(a, nitem) + lane : gp;
            scan16_group_scores(acc, ring, gp, np, qb, QTr, K4);

            // a group none of whose scores exceeds its query's radius emits nothing: the common case
            // (a NaN score or radius compares false; rows past n_rows that pass are masked below)
            bool anyp = false;
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) anyp |= (acc[rr] > rad);
            if (__any(anyp)) {
                const int nvalid = rows_valid(a.n_rows, g);
                u32 tot = 0;   // wave-uniform: the wave's hits in this group
#pragma unroll
                for (int rr = 0; rr < 16; ++rr) tot += (u32)__popcll(__ballot(acc[rr] > rad && scan16_row(rr, lane) < nvalid));
                if (tot != 0u) {
                    // one atomic per wave and group: the wave's pairs are a dense run of the staging buffer, a lane's slot
                    // is the run's start + the hits before it (ballot + prefix)
                    u64 start = 0;
                    if (lane == 0) start = atomicAdd(reinterpret_cast<unsigned long long *>(ra.cursor), (unsigned long long)tot);
                    const u32 s_lo = (u32)__builtin_amdgcn_readfirstlane((int)(u32)start);
                    const u32 s_hi = (u32)__builtin_amdgcn_readfirstlane((int)(u32)(start >> 32));
                    start = ((u64)s_hi << 32) | s_lo;
                    const u64 below = (1ull << lane) - 1ull;
                    const u32 qg = ra.q_base + (u32)(q0 + jc);
                    u32 base = 0;
#pragma unroll
                    for (int rr = 0; rr < 16; ++rr) {
                        const int row = scan16_row(rr, lane);
                        const float s = acc[rr];
                        const bool hit = s > rad && row < nvalid;
                        const u64 vote = __ballot(hit);
                        if (hit) {
                            const u64 at = start + base + (u32)__popcll(vote & below);
                            if (at < ra.cap) {   // counting never stops; what does not fit is dropped
                                ra.stage_key[at] = make_key(s, g * GROUP_ROWS + row);
                                ra.stage_q[at] = qg;
                            }
                            cnt += 1u;
                        }
                        base += (u32)__popcll(vote);
                    }
                }
            }
        }
        item = nitem;
        have = have_next;
    }

    // the four lane groups of a wave that share a query, then the waves, then one integer atomic per (workgroup, query)
    u32 c = cnt;
    c += (u32)__shfl_xor((int)c, 16);
    c += (u32)__shfl_xor((int)c, 32);
    if (lane < 16) red[w * 16 + lane] = c;
    __syncthreads();
    if (tid < QTr) {
        u64 sum = 0;
#pragma unroll
        for (int ww = 0; ww < SCAN_WAVES; ++ww) sum += red[ww * 16 + tid];
        if (sum != 0ull) atomicAdd(reinterpret_cast<unsigned long long *>(&ra.counts[q0 + tid]), (unsigned long long)sum);
    }
}

// One workgroup.  lims[i] = counts[0] + .. + counts[i - 1], lims[nq] = the total; blk likewise over the segments' blocks of
// RANGE_SORT_N keys (what range_sort_kernel and range_merge_kernel find their work by); the scatter's cursors are zeroed;
// ctl[RANGE_TOTAL], ctl[RANGE_FITS].  A thread sums a contiguous run of queries, the 256 sums are scanned in LDS.
__global__ __launch_bounds__(RANGE_THREADS) void range_offsets_kernel(const u64 *__restrict__ counts, long nq, u64 cap, u64 *__restrict__ ctl,
                                                                      long long *__restrict__ lims, u32 *__restrict__ blk, u32 *__restrict__ qcur) {
    __shared__ u64 part_c[RANGE_THREADS];
    __shared__ u64 part_b[RANGE_THREADS];
    const int tid = threadIdx.x;
    const long per = (nq + RANGE_THREADS - 1) / RANGE_THREADS;
    const long lo = min(nq, tid * per), hi = min(nq, lo + per);
    u64 sc = 0, sb = 0;
    for (long i = lo; i < hi; ++i) {
        const u64 c = counts[i];
        sc += c;
        sb += (c + RANGE_SORT_N - 1) / RANGE_SORT_N;
    }
    part_c[tid] = sc;
    part_b[tid] = sb;
    __syncthreads();
    u64 oc = 0, ob = 0;
    for (int t = 0; t < tid; ++t) {
        oc += part_c[t];
        ob += part_b[t];
    }
    for (long i = lo; i < hi; ++i) {
        const u64 c = counts[i];
        lims[i] = (long long)oc;
        blk[i] = (u32)ob;   // (meaningful when the result fits: then the blocks are fewer than cap / RANGE_SORT_N + nq)
        qcur[i] = 0u;
        oc += c;
        ob += (c + RANGE_SORT_N - 1) / RANGE_SORT_N;
    }
    if (tid == RANGE_THREADS - 1) {   // (its run is the last one, or empty behind the last one: oc, ob are the totals)
        lims[nq] = (long long)oc;
        blk[nq] = (u32)ob;
        ctl[RANGE_TOTAL] = oc;
        ctl[RANGE_FITS] = oc <= cap ? 1ull : 0ull;
    }
}

// staged pair -> the next free slot of its query's segment; the order inside a segment is fixed by the sort
__global__ __launch_bounds__(RANGE_THREADS) void range_scatter_kernel(const u64 *__restrict__ ctl, const u64 *__restrict__ stage_key,
                                                                      const u32 *__restrict__ stage_q, const long long *__restrict__ lims,
                                                                      u32 *__restrict__ qcur, u64 *__restrict__ keys) {
    if (ctl[RANGE_FITS] == 0ull) return;
    const u64 i = (u64)blockIdx.x * RANGE_THREADS + threadIdx.x;
    if (i >= ctl[RANGE_TOTAL]) return;
    const u32 q = stage_q[i];
    const u32 at = atomicAdd(&qcur[q], 1u);
    keys[(u64)lims[q] + at] = stage_key[i];
}

// workgroup w of the block-numbered grids -> (query, block inside its segment): the last query with blk[q] <= w
__device__ __forceinline__ long range_find_block(const u32 *__restrict__ blk, long nq, u32 w) {
    long lo = 0, hi = nq - 1;
    while (lo < hi) {
        const long mid = (lo + hi + 1) >> 1;
        if (blk[mid] <= w) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}
// merge passes a segment of nb blocks needs: ceil(log2(nb))
__device__ __forceinline__ int range_passes_of(u32 nb) { return nb <= 1u ? 0 : 32 - __clz((int)(nb - 1u)); }

// Workgroup = one block of <= RANGE_SORT_N keys of one segment: sorted descending in LDS.  A segment that needs k of the call's
// `passes` merge passes takes part in the last k of them, so its sorted blocks go to the buffer pass number (passes - k) reads:
// every segment ends in the buffer the last pass writes, without a copy.  bufs[0] is where the scatter left the keys.
__global__ __launch_bounds__(RANGE_THREADS) void range_sort_kernel(const u64 *__restrict__ ctl, const long long *__restrict__ lims,
                                                                   const u32 *__restrict__ blk, long nq, int passes, u64 *__restrict__ buf0,
                                                                   u64 *__restrict__ buf1) {
    __shared__ u64 buf[RANGE_SORT_N];
    if (ctl[RANGE_FITS] == 0ull) return;
    const u32 w = blockIdx.x;
    if (w >= blk[nq]) return;
    const int tid = threadIdx.x;
    const long q = range_find_block(blk, nq, w);
    const u64 seg0 = (u64)lims[q], len = (u64)lims[q + 1] - seg0;
    const u64 off = (u64)(w - blk[q]) * RANGE_SORT_N;
    const u32 n = (u32)min((u64)RANGE_SORT_N, len - off);
    const int k = range_passes_of(blk[q + 1] - blk[q]);
    u64 *dst = ((passes - k) & 1) ? buf1 : buf0;
    for (u32 i = tid; i < n; i += RANGE_THREADS) buf[i] = buf0[seg0 + off + i];
    __syncthreads();
    if (n > 1) block_sort_desc(buf, n, tid, RANGE_THREADS);
    for (u32 i = tid; i < n; i += RANGE_THREADS) dst[seg0 + off + i] = buf[i];
}

// first x outputs of the merge of two descending runs with unique keys: how many come from a
__device__ __forceinline__ u64 range_merge_split(const u64 *__restrict__ a, u64 la, const u64 *__restrict__ b, u64 lb, u64 x) {
    u64 lo = x > lb ? x - lb : 0, hi = x < la ? x : la;
    while (lo < hi) {
        const u64 mid = (lo + hi) >> 1;
        if (a[mid] > b[x - 1 - mid]) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// Merge pass `pass` of `passes`: src holds sorted runs, dst gets runs twice as long.  Workgroup = one tile of RANGE_SORT_N
// outputs of one segment (numbered like the sort's blocks).  A segment that needs k passes joins at pass passes - k with runs
// of RANGE_SORT_N; before that its workgroups exit.  The tile's inputs (merge path: one binary search per tile end) go to LDS,
// every key's place in the tile is its index in its own run + the keys of the other run ahead of it.
__global__ __launch_bounds__(RANGE_THREADS) void range_merge_kernel(const u64 *__restrict__ ctl, const long long *__restrict__ lims,
                                                                    const u32 *__restrict__ blk, long nq, int passes, int pass,
                                                                    const u64 *__restrict__ src, u64 *__restrict__ dst) {
    __shared__ u64 buf[RANGE_SORT_N];
    __shared__ u64 split[2];
    if (ctl[RANGE_FITS] == 0ull) return;
    const u32 w = blockIdx.x;
    if (w >= blk[nq]) return;
    const int tid = threadIdx.x;
    const long q = range_find_block(blk, nq, w);
    const int k = range_passes_of(blk[q + 1] - blk[q]);
    if (pass < passes - k) return;
    const u64 seg0 = (u64)lims[q], len = (u64)lims[q + 1] - seg0;
    const u64 R = (u64)RANGE_SORT_N << (pass - (passes - k));
    const u64 o0 = (u64)(w - blk[q]) * RANGE_SORT_N;   // the tile's first output, inside the segment
    const u64 ps = o0 / (2 * R) * (2 * R);             // the pair of runs it belongs to: a = [ps, a1), b = [a1, b1)
    const u64 a1 = min(ps + R, len), b1 = min(ps + 2 * R, len);
    const u64 la = a1 - ps, lb = b1 - a1;
    const u64 *a = src + seg0 + ps, *b = src + seg0 + a1;
    const u64 x0 = o0 - ps, x1 = min(x0 + RANGE_SORT_N, la + lb);
    if (tid == 0) split[0] = range_merge_split(a, la, b, lb, x0);
    if (tid == 64) split[1] = range_merge_split(a, la, b, lb, x1);
    __syncthreads();
    const u64 ia0 = split[0], ia1 = split[1], ib0 = x0 - ia0, ib1 = x1 - ia1;
    const u32 na = (u32)(ia1 - ia0), nb = (u32)(ib1 - ib0);   // na + nb = x1 - x0 <= RANGE_SORT_N
    u64 *sa = buf, *sb = buf + na;
    for (u32 i = tid; i < na; i += RANGE_THREADS) sa[i] = a[ia0 + i];
    for (u32 i = tid; i < nb; i += RANGE_THREADS) sb[i] = b[ib0 + i];
    __syncthreads();
    u64 *out = dst + seg0 + o0;
    for (u32 i = tid; i < na + nb; i += RANGE_THREADS) {
        const bool from_a = i < na;
        const u32 own = from_a ? i : i - na;
        const u64 key = buf[i];
        const u64 *other = from_a ? sb : sa;
        u32 lo = 0, hi = from_a ? nb : na;   // keys of the other run ahead of this one: the first index whose key is smaller
        while (lo < hi) {
            const u32 mid = (lo + hi) >> 1;
            if (other[mid] > key) lo = mid + 1;
            else hi = mid;
        }
        out[own + lo] = key;
    }
}

// keys -> (D, I) in [0, lims[nq]); nothing behind it is written, and nothing at all when the result does not fit
__global__ __launch_bounds__(RANGE_THREADS) void range_results_kernel(const u64 *__restrict__ ctl, const u64 *__restrict__ keys,
                                                                      const long long *__restrict__ id_map, float *__restrict__ D,
                                                                      long long *__restrict__ I) {
    if (ctl[RANGE_FITS] == 0ull) return;
    const u64 i = (u64)blockIdx.x * RANGE_THREADS + threadIdx.x;
    if (i >= ctl[RANGE_TOTAL]) return;
    const u64 key = keys[i];
    const u32 pos = 0xFFFFFFFFu - (u32)key;
    D[i] = ord2f((u32)(key >> 32));
    I[i] = id_map ? id_map[pos] : (long long)pos;
}
