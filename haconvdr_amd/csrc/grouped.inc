// Search by group (hac_index_search_grouped*): included by flat_ip.hip.
//
// grouped(q, g, k) = the first k of { rep(q, G) : G a label that occurs } by (score desc, row asc), rep(q, G) = the row of group G
// with the greatest key among its rows whose score is not NaN.  Labels are int64 [n_rows] with values in [0, 2^32); a row whose
// label lies outside that range is in no list (the device forms' rule; the host form has refused it).  Two kernels:
// scan16_grouped_kernel is scan16_kernel with candidate lists that are de-duplicated by label every time they are compacted;
// grouped_select_kernel reduces the workgroups' survivors of a query (or the shards' lists of a multi-device index) to the
// best key of every label, cut at k.
struct GroupArgs {
    const long long *group_of;   // [n_labels] the label of row (position - pos_base)
    long n_labels;
    u32 pos_base;                // position of label 0's row (0 everywhere today)
};
typedef const __attribute__((address_space(1))) long long *gi64ptr;

// (label << 32) | (0xFFFFFFFF - i) of the key at list position i, or 0: the key names no row with a label in [0, 2^32).  A word
// is never 0 otherwise (i < 2^32 - 1), and sorted descending the words of one label are adjacent, the best list position first.
__device__ __forceinline__ u64 label_word(const GroupArgs &g, u64 key, u32 i) {
    const u32 pos = 0xFFFFFFFFu - (u32)key;
    const long local = (long)pos - (long)g.pos_base;
    if (key == 0ull || local < 0 || local >= g.n_labels) return 0ull;   // no address from a slot that holds no row
    const long long lab = ((gi64ptr)g.group_of)[local];
    if (lab < 0 || lab > 0xFFFFFFFFll) return 0ull;
    return ((u64)lab << 32) | (u64)(0xFFFFFFFFu - i);
}

// One wave: buf[0, n) (any order, n <= capacity of buf and scr, both powers of two) -> the best key of every label, sorted
// descending, in buf[0, m'), m' = min(m, k), m the number of distinct labels; returns m, or some value >= k when m >= k (buf[k - 1]
// is then the k-th best group's key).  Sort the keys; sort the label words; a word that is not the first of its label's run names a key that a better
// key of the same label beats: zero it, and the keys without a label with it; then close the gaps in order (a lane per key,
// ballot + prefix: a destination never lies behind its source, and a chunk is read before any of its lanes stores).
__device__ u32 wave_dedup(u64 *buf, u64 *scr, u32 n, u32 k, const GroupArgs &g, int lane) {
    wave_sort_desc(buf, n, lane);
    for (u32 i = lane; i < n; i += 64) {
        const u64 wd = label_word(g, buf[i], i);
        if (wd == 0ull) buf[i] = 0ull;   // OUT-OF-RANGE LABELS GO BEFORE THE DEDUP
        scr[i] = wd;
    }
    lds_fence();
    wave_sort_desc(scr, n, lane);
    for (u32 t = lane; t < n; t += 64) {
        const u64 wd = scr[t];
        if (t > 0 && wd != 0ull && (scr[t - 1] >> 32) == (wd >> 32)) buf[0xFFFFFFFFu - (u32)wd] = 0ull;   // (a list position < n)
    }
    lds_fence();
    const u64 below = (1ull << lane) - 1ull;
    u32 m = 0;
    // (n, k and m are equal in every lane by their VALUES -- the caller keeps k in a vector register, so the compiler treats this loop and
    // the caller's `n > hwv` as divergent; every lane takes them alike and the ballot sees the whole wave)
    for (u32 base = 0; base < n && m < k; base += 64) {   // wave-uniform; m >= k is all the caller asks once k keys stand
        const u32 i = base + lane;
        const u64 key = i < n ? buf[i] : 0ull;
        const bool keep = key != 0ull;
        const u64 vote = __ballot(keep);
        const u32 at = m + (u32)__popcll(vote & below);
        if (keep && at < k) buf[at] = key;
        m += (u32)__popcll(vote);
    }
    lds_fence();
    return m;
}

// scan16_kernel with per-label candidate lists.  Workgroup = (row stream blockIdx.x, tile of <= QT queries blockIdx.y); uses
// a.segs, a.nseg, a.q, a.nq, a.K4, a.k, a.C, a.QT, a.n_rows, a.n_items, a.thr_glob, a.partial, a.partial_cnt, a.pos_base of
// ScanArgs (a.thr_init is not read: there is no seeding and no fp16 prefilter, a sample of rows says nothing about groups).
// Built from scan16_core.inc as scan16_kernel is: scan16_stage_queries, scan16_group_scores, scan16_row / rows_valid; the
// row-stream cursor and the append epilogue are its own copies of scan16_kernel's, the compaction round and the flush are its
// own dedup variants.  LDS: scan16's, plus one scratch array u64 [C] per compacting wave ([min(SCAN_WAVES, QTr)][C]).  What
// must hold here:
//   DEDUP BEFORE THRESHOLD  a threshold is the k-th key of a compaction that left k DISTINCT labels: the k-th best of k distinct
//       groups' entries, hence a proven lower bound of the k-th group score (every group's representative is at least its entry).
//       A row below it can be no group's representative in the answer.  A threshold only filters such rows, so the result does
//       not depend on the row streams P, on where the launches are cut or on the order of work.
//   cnt <= k AFTER EVERY COMPACTION  the invariant C >= k + 64 * SCAN_WAVES rests on: a buffer full of one group's rows shrinks
//       to one entry and the scan goes on, with no threshold.
//   NO GLOBAL BEST IS DROPPED  a compaction drops a key only under a better key of its own label (it is then not the
//       representative) or under k better keys of k distinct other labels (their groups' representatives are at least as good:
//       its group is not in the answer through this row).
//   OUT-OF-RANGE LABELS  (device form) rows with such a label are zeroed in the compaction before the dedup, and at the final
//       flush, which compacts every list once more: no such row reaches a threshold or the survivors.
//   NO ADDRESS FROM A DEAD SLOT  a label is read only for a non-empty key whose row lies in [0, n_labels); UNIFORM BARRIERS
//       nrounds comes from a.n_items and gridDim, which every wave reads alike; the compactions are per wave and use fences only.
__global__ __launch_bounds__(SCAN_WAVES * 64) void scan16_grouped_kernel(ScanArgs a, GroupArgs gr) {
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
    u64 *scratch = cand + (size_t)QTr * C;                                 // [min(SCAN_WAVES, QTr)][C]: wave w's, when it owns a query
    u32 *cnt = reinterpret_cast<u32 *>(scratch + (size_t)min(SCAN_WAVES, QTr) * C);   // [16]
    float *thr = reinterpret_cast<float *>(cnt + 16);                      // [16]
    u64 *scr = scratch + (size_t)min(w, QTr - 1) * C;

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

    // Uniform values that only the epilogue and the compactions use live in vector registers: this kernel has the labels and the
    // scratch array more than scan16_kernel to keep in scalar ones, which are full there (no spills; scan16_filter.inc does the same)
    u32 pos_base = a.pos_base;
    u32 *tglob = a.thr_glob + q0;
    GroupArgs grv = gr;
    u32 kk = (u32)a.k, hwv = hw;
    long n_rows = a.n_rows;
    asm volatile("" : "+v"(pos_base), "+v"(tglob), "+v"(grv.group_of), "+v"(grv.n_labels), "+v"(grv.pos_base), "+v"(scr), "+v"(kk), "+v"(hwv), "+v"(n_rows));

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
            for (int rr = 0; rr < 16; ++rr) anyp |= (acc[rr] >= th);
            if (__any(anyp)) {
                const int nvalid = rows_valid(n_rows, g);
                if (j < QTr) {
#pragma unroll
                    for (int rr = 0; rr < 16; ++rr) {
                        const int row = scan16_row(rr, lane);
                        const float s = acc[rr];
                        if (s >= th && row < nvalid) {   // (a NaN score fails s >= th: th is -inf or a score)
                            const u32 pos = atomicAdd(&cnt[j], 1u);
                            cand[(size_t)j * C + pos] = make_key(s, pos_base + g * GROUP_ROWS + row);
                        }
                    }
                }
            }
        }
        __syncthreads();  // (B) all appends of this round are visible
        for (int jj = w; jj < QTr; jj += SCAN_WAVES) {
            const u32 n = cnt[jj];
            float t_new = -INFINITY;
            u32 m = 0;
            if (n > hwv) {  // wave-uniform
                m = wave_dedup(cand + (size_t)jj * C, scr, n, kk, grv, lane);
                // DEDUP BEFORE THRESHOLD: only k distinct labels make one
                if (m >= kk) t_new = ord2f((u32)(cand[(size_t)jj * C + kk - 1] >> 32));
            }
            if (lane == 0) {
                float t_cur = thr[jj];
                if (n > hwv) {
                    cnt[jj] = min(m, kk);   // cnt <= k AFTER EVERY COMPACTION
                    if (t_new > t_cur) {
                        t_cur = t_new;
                        atomicMax(&tglob[jj], f2ord(t_new));
                    }
                }
                const u32 go = __hip_atomic_load(&tglob[jj], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (go != 0u) t_cur = fmaxf(t_cur, ord2f(go));
                thr[jj] = t_cur;
            }
        }
        item = nitem;
        have = have_next;
    }

    __syncthreads();
    for (int jj = w; jj < QTr; jj += SCAN_WAVES) {
        u32 n = cnt[jj];
        u64 *b = cand + (size_t)jj * C;
        // the list goes out as the best key of each of its labels, at most k (flush_survivors then neither sorts nor cuts)
        if (n > 0) n = min(wave_dedup(b, scr, n, kk, grv, lane), kk);
        flush_survivors(a, gridDim.x, q0 + jj, b, n, lane);
    }
}

// One workgroup per query: the best key of every label among the query's input keys, sorted, cut at k -> out [nq][k], 0-padded.
//   dense input (counts != null): min(counts[q], cap) keys at lists[q * stride_q ..], the survivors a scan appended;
//   slab input  (counts == null): L lists of k keys, element (l, q, i) at lists[l * stride_l + q * stride_q + i]: the shards'
//   lists of a multi-device index, positions already those of the whole index, g.group_of the whole label array.
// The keys stream through an LDS buffer of Cm (a power of two >= k + 256) 256 at a time; a full buffer is sorted, reduced to its
// labels' best keys and cut at k (block_dedup: wave_dedup's two sorts by the workgroup, and a third sort of the keys where the wave closes the gaps
// with an ordered ballot pass), and with k distinct labels its k-th key
// becomes a filter for the rest of the stream -- the scan's DEDUP BEFORE THRESHOLD argument, on keys.  No atomics: a key's slot
// is a ballot prefix, and the output is a pure function of the input SET (keys are unique: a row is scored once).
// Dynamic LDS: 2 * Cm * 8 bytes.
__device__ u32 block_dedup(u64 *buf, u64 *scr, u32 n, const GroupArgs &g, int tid) {
    block_sort_desc(buf, n, tid, 256);
    for (u32 i = tid; i < n; i += 256) {
        const u64 wd = label_word(g, buf[i], i);
        if (wd == 0ull) buf[i] = 0ull;
        scr[i] = wd;
    }
    __syncthreads();
    block_sort_desc(scr, n, tid, 256);
    for (u32 t = tid; t < n; t += 256) {
        const u64 wd = scr[t];
        if (t > 0 && wd != 0ull && (scr[t - 1] >> 32) == (wd >> 32)) buf[0xFFFFFFFFu - (u32)wd] = 0ull;
    }
    __syncthreads();
    block_sort_desc(buf, n, tid, 256);   // the zeros sink behind the m kept keys
    u32 lo = 0, hi = n;                  // m = the first empty slot (every thread finds the same)
    while (lo < hi) {
        const u32 mid = (lo + hi) >> 1;
        if (buf[mid] != 0ull) lo = mid + 1;
        else hi = mid;
    }
    __syncthreads();
    return lo;
}

__global__ __launch_bounds__(256) void grouped_select_kernel(const u64 *__restrict__ lists, int L, size_t stride_l, size_t stride_q, const u32 *__restrict__ counts,
                                                             u32 cap, int k, int Cm, GroupArgs g, u64 *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u64 *buf = reinterpret_cast<u64 *>(smem);   // [Cm]
    u64 *scr = buf + Cm;                        // [Cm]
    __shared__ u32 wsum[4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const size_t q = blockIdx.x;
    const u64 below = (1ull << lane) - 1ull;
    const long total = counts ? (long)min(counts[q], cap) : (long)L * k;
    u32 n = 0;         // keys in buf (workgroup-uniform)
    u64 thrk = 0ull;   // with k distinct labels seen: the k-th of their best keys
    for (long base = 0; base < total; base += 256) {
        const long idx = base + tid;
        u64 key = 0ull;
        if (idx < total) {
            if (counts) {
                key = lists[q * stride_q + idx];
            } else {
                const long l = idx / k;
                key = lists[(size_t)l * stride_l + q * stride_q + (size_t)(idx - l * k)];
            }
        }
        const bool keep = key != 0ull && key > thrk;   // (the k-th key itself is in buf already)
        const u64 vote = __ballot(keep);
        if (lane == 0) wsum[w] = (u32)__popcll(vote);
        __syncthreads();
        u32 at = n + (u32)__popcll(vote & below), all = 0;
        for (int ww = 0; ww < 4; ++ww) {
            const u32 c = wsum[ww];
            if (ww < w) at += c;
            all += c;
        }
        if (keep) buf[at] = key;   // at < n + 256 <= Cm
        n += all;
        __syncthreads();
        if (n > (u32)(Cm - 256)) {   // uniform
            const u32 m = block_dedup(buf, scr, n, g, tid);
            n = min(m, (u32)k);
            if (m >= (u32)k) thrk = buf[k - 1];
            __syncthreads();
        }
    }
    if (n > 0) n = min(block_dedup(buf, scr, n, g, tid), (u32)k);
    for (u32 i = tid; i < (u32)k; i += 256) out[q * k + i] = i < n ? buf[i] : 0ull;
}

// keys -> (D, I, G); empty slots: -FLT_MAX / -1 / -1.  G (optional) is the row's own label, never id_map's value.
__global__ void grouped_results_kernel(const u64 *__restrict__ keys, long n, const long long *__restrict__ id_map, GroupArgs g, float *__restrict__ D,
                                       long long *__restrict__ I, long long *__restrict__ G) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u64 key = keys[i];
    if (key == 0ull) {
        D[i] = -FLT_MAX;
        I[i] = -1;
        if (G) G[i] = -1;
    } else {
        const u32 pos = 0xFFFFFFFFu - (u32)key;
        D[i] = ord2f((u32)(key >> 32));
        I[i] = id_map ? id_map[pos] : (long long)pos;
        if (G) G[i] = (long)pos < g.n_labels ? g.group_of[pos] : -1ll;
    }
}
