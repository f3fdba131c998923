// Entry at a rank (hac_index_entries_at*): included by flat_ip.hip.
//
// entry_at(q, t) = the t-th key (0-based) of { make_key(s(q, r), pos_base + r) : r in [0, n_rows), s(q, r) not NaN } in
// descending order -- the inverse of count_ahead.  A radix selection over the 64-bit key, from the top digit down, per (query,
// rank) PAIR: a pair carries the key prefix found so far and the rank that remains inside it.  One pass over the corpus per
// digit: rank_hist_kernel counts, per pair, the rows whose higher digits equal the prefix by the value of the digit;
// rank_narrow_kernel then walks the pair's bins from the top, finds the one that holds the remaining rank, extends the prefix by
// it and subtracts the rows above.  After the last digit the prefix is the key.  Nothing is collected and nothing can overflow:
// no pass bound, nothing for the status ring, and the launches depend on the shape of the call and the index's size only.
//
// A pair takes one query slot of a 16-wide tile: a query asked for m ranks appears m times (the stated cost model: the corpus is
// streamed once per digit and tile of 16 pairs).  Position digits that cannot differ among the index's rows are not selected:
// the host fills them into the prefix (rows_host.inc: at_rank_digits).
struct AtState {
    u64 prefix;      // the key's digits found so far, the others zero (position digits no row differs in: set from the start)
    long long rem;   // the rank that remains among the rows matching the prefix; < 0: a dead pair (rank outside the list), key 0
};
struct AtArgs {
    const AtState *state;   // [pairs of this launch]; not read by the first pass
    u32 *hist;              // [pairs of this launch][BINS], zero before the pass
    long m;                 // ranks per query: the launch's pair p asks query (pair0 + p) / m
    long pair0;             // the launch's first pair in the call's [nq][m] matrix
    int shift;              // the digit's lowest bit: 64 - BITS (the first pass) .. 0
};

constexpr int AT_BITS = 8;
// dynamic LDS: queries [K4][QT] f4, histograms u32 [16][BINS], prefixes u64 [16], live flags u32 [16]
constexpr size_t at_rank_lds(int K4, int QT, int BITS) { return (size_t)K4 * QT * 16 + (size_t)16 * 4 * (1u << BITS) + 16 * 8 + 16 * 4; }

// Workgroup = (row stream blockIdx.x, tile of <= 16 pairs blockIdx.y).  Uses a.segs, a.nseg, a.q (the queries of the whole
// call), a.nq (the PAIRS of this launch), a.K4, a.QT, a.n_rows, a.n_items (groups, from group 0), a.pos_base of ScanArgs.
// Built from scan16_core.inc as count_ahead_kernel is: scan16_stage_queries (a slot's row of a.q is its pair's query),
// scan16_group_scores, scan16_row / rows_valid; the row-stream cursor is written out here.
// The epilogue: every (pair, row) with a non-NaN score and row < n_rows whose key agrees with the pair's prefix above the digit
// adds 1 to bin digit(key) of the pair's histogram in LDS; the workgroup's histograms go to global memory with one integer
// atomic per non-empty bin.  Integer sums: the result is a pure function of the inputs, whatever P, the launch cuts, the order.
//   GATE  behind the first digit a group is looked at only if one of its scores agrees with a live pair's prefix in the score
//       bits found so far (a test on the ordered score word, in front of the u64 one that decides); after one or two digits
//       almost no group does.
//   CONTENTION  the top digit of real scores (sign and high exponent bits) is nearly constant: a lane sums the run of equal
//       digits along its 16 rows in a register and issues one LDS atomic per run -- one per group in the common case, not 16.
template <int BITS>
__global__ __launch_bounds__(SCAN_WAVES * 64) void rank_hist_kernel(ScanArgs a, AtArgs ra) {
    static_assert(64 % BITS == 0 && 32 % BITS == 0, "digits must not straddle the score / position words");
    constexpr int BINS = 1 << BITS;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int K4 = a.K4;
    const int q0 = blockIdx.y * a.QT;
    const int QTr = min(a.QT, a.nq - q0);
    const int shift = ra.shift;
    const bool first = shift == 64 - BITS;
    const int hs = shift + BITS;   // the bits below the digits already found

    f4 *ldsQ = reinterpret_cast<f4 *>(smem);                                   // [K4][QTr]
    u32 *hist = reinterpret_cast<u32 *>(smem + (size_t)K4 * a.QT * 16);         // [16][BINS]
    u64 *pfx = reinterpret_cast<u64 *>(hist + 16 * BINS);                       // [16]
    u32 *alive = reinterpret_cast<u32 *>(pfx + 16);                             // [16]

    scan16_stage_queries(ldsQ, a.q, K4, QTr, tid, [&](int j) { return (ra.pair0 + q0 + j) / ra.m; });   // the pair's query
    for (int i = tid; i < 16 * BINS; i += SCAN_WAVES * 64) hist[i] = 0u;
    if (tid < 16) {
        bool live = tid < QTr;
        u64 p = 0ull;
        if (live && !first) {
            const AtState s = ra.state[q0 + tid];
            live = s.rem >= 0;
            p = s.prefix;
        }
        pfx[tid] = p;
        alive[tid] = live ? 1u : 0u;
    }
    __syncthreads();

    const int j = lane & 15;
    const int jc = min(j, QTr - 1);
    const f4 *qb = ldsQ + jc;
    const u32 stride = gridDim.x * SCAN_WAVES;
    const u32 nrounds = (a.n_items + stride - 1) / stride;
    const bool live = alive[j] != 0u;
    const u64 prefix = pfx[j];
    const u32 phi = (u32)(prefix >> 32);
    const int osh = hs >= 32 ? hs - 32 : 0;   // (first pass: not used)

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

            // GATE (a NaN score may pass it: the epilogue drops it; rows past n_rows that pass are masked below)
            bool anyp = live && first;
            if (!first) {
#pragma unroll
                for (int rr = 0; rr < 16; ++rr) anyp |= ((f2ord(acc[rr] + 0.0f) ^ phi) >> osh) == 0u;
                anyp = anyp && live;
            }
            if (__any(anyp)) {
                const int nvalid = rows_valid(a.n_rows, g);
                if (live) {
                    u32 cd = 0u, cc = 0u;   // CONTENTION: the run of equal digits so far
#pragma unroll
                    for (int rr = 0; rr < 16; ++rr) {
                        const int row = scan16_row(rr, lane);
                        const float s = acc[rr];
                        if (s == s && row < nvalid) {
                            const u64 key = make_key(s, a.pos_base + g * GROUP_ROWS + row);
                            if (first || ((key ^ prefix) >> hs) == 0ull) {
                                const u32 dg = (u32)(key >> shift) & (u32)(BINS - 1);
                                if (dg != cd && cc != 0u) {
                                    atomicAdd(&hist[j * BINS + cd], cc);
                                    cc = 0u;
                                }
                                cd = dg;
                                ++cc;
                            }
                        }
                    }
                    if (cc != 0u) atomicAdd(&hist[j * BINS + cd], cc);
                }
            }
        }
        item = nitem;
        have = have_next;
    }

    // the workgroup's histograms: one integer atomic per non-empty bin of a pair of the tile.  A bin holds at most n_rows
    // <= 2^32 - 1 rows: u32 counters cannot wrap.
    __syncthreads();
    for (int i = tid; i < QTr * BINS; i += SCAN_WAVES * 64) {
        const u32 v = hist[i];
        if (v != 0u) atomicAdd(&ra.hist[(size_t)q0 * BINS + i], v);
    }
}

// Between two passes, one wave per pair: the bins from the top, the one that holds the remaining rank, the prefix extended, the
// rows above it subtracted; the histogram is left zero for the next pass.  The first pass (shift == 64 - BITS) starts the
// pair: prefix = const_bits (the position digits no row of the index differs in), remaining rank = ranks[pair]; a rank < 0 or
// >= the total -- the number of listable rows, |L(q)| -- marks the pair dead.  keys_out != null (the last pass): the prefix
// is the key; a dead pair's is 0.
template <int BITS>
__global__ __launch_bounds__(64) void rank_narrow_kernel(u32 *__restrict__ hist, AtState *__restrict__ state, const long long *__restrict__ ranks,
                                                         int shift, u64 const_bits, u64 *__restrict__ keys_out) {
    constexpr int BINS = 1 << BITS, PER = BINS / 64;
    static_assert(BINS % 64 == 0, "a lane owns BINS / 64 bins");
    const long pair = blockIdx.x;
    const int lane = threadIdx.x;
    u32 *h = hist + (size_t)pair * BINS;
    // lane l owns the bins BINS - 1 - PER * l downwards: lane order == descending digit order
    u32 c[PER];
    u64 loc = 0;
#pragma unroll
    for (int t = 0; t < PER; ++t) {
        const int bin = BINS - 1 - (PER * lane + t);
        c[t] = h[bin];
        h[bin] = 0u;
        loc += c[t];
    }
    u64 incl = loc;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const u64 v = __shfl_up(incl, off);
        if (lane >= off) incl += v;
    }
    const u64 total = __shfl(incl, 63);
    const u64 excl = incl - loc;

    AtState s;
    if (shift == 64 - BITS) {
        s.prefix = const_bits;
        s.rem = ranks[pair];
    } else {
        s = state[pair];
    }
    // (behind the first pass a live pair's rank is inside its prefix's rows by construction; if it were not, the pair dies)
    const bool dead = s.rem < 0 || (u64)s.rem >= total;
    if (dead) {
        if (lane == 0) {
            state[pair] = AtState{0ull, -1ll};
            if (keys_out) keys_out[pair] = 0ull;
        }
        return;
    }
    const u64 want = (u64)s.rem;
    if (want >= excl && want < incl) {   // exactly one lane
        u64 r = want - excl;
        int t_hit = 0;
        bool found = false;
#pragma unroll
        for (int t = 0; t < PER; ++t) {
            if (!found) {
                if (r < (u64)c[t]) {
                    found = true;
                    t_hit = t;
                } else {
                    r -= c[t];
                }
            }
        }
        const u64 bin = (u64)(BINS - 1 - (PER * lane + t_hit));
        const u64 p = s.prefix | (bin << shift);
        state[pair] = AtState{p, (long long)r};
        if (keys_out) keys_out[pair] = p;
    }
}
