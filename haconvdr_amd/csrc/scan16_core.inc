// The parts scan16_kernel and the kernels of its shape are built from: included by flat_ip.hip in front of scan16_kernel.
// (scan16_filter.inc's body -- scan16_masked_kernel, scan16_after_kernel, scan16_masked_after_kernel --, scan16_grouped_kernel,
// count_ahead_kernel, range_emit_kernel, rank_hist_kernel.)
// Forced-inline device functions only: every kernel keeps its own __global__ function and its own register allocation, and the
// chunk loop each one compiles to is the one it had when the loop was written out in it.
// Not here, on purpose (LABNOTES, "One shared row loop"): the row-stream cursor (item, have, nitem, have_next, np) -- written
// as one function that takes the round as a callable it cost scan16_after_kernel, scan16_grouped_kernel and rank_hist_kernel
// 14 to 16 VGPRs each, by value and by reference alike, so every body spells it out -- and the append epilogues, whose
// BEFORE APPEND rules read best as the dozen lines they are.  (The three filtered kernels share cursor and epilogue as ONE
// body with two compile-time questions, scan16_filter.inc: a whole body instantiated three times, not a callable.)
//
// A wave scores one T64 group (64 rows, lane l streams row l's chunks) against the <= 16 queries of its tile with
// v_mfma_f32_16x16x1: accumulator slot rr of lane l is the score of row scan16_row(rr, l) and query l & 15.

// the row (of its group) whose score accumulator slot rr of this lane holds
__device__ __forceinline__ int scan16_row(int rr, int lane) { return 16 * (rr >> 2) + 4 * (lane >> 4) + (rr & 3); }

// the rows of group g that exist; the rows behind them are zeros, or stale after reset() + a smaller add()
__device__ __forceinline__ int rows_valid(long n_rows, u32 g) {
    const long rem = n_rows - (long)g * GROUP_ROWS;
    return rem < GROUP_ROWS ? (int)rem : GROUP_ROWS;
}

// The query tile into LDS as [K4][QTr] f4, by the whole workgroup (the caller's barrier follows).  row_of(j) is the row of q
// that slot j of the tile scores: q0 + j, or the query of a (query, rank) pair.
template <class RowOf>
__device__ __forceinline__ void scan16_stage_queries(f4 *ldsQ, const float4 *q, int K4, int QTr, int tid, RowOf row_of) {
    for (int idx = tid; idx < K4 * QTr; idx += SCAN_WAVES * 64) {
        const int k4 = idx / QTr, j = idx - k4 * QTr;
        ldsQ[idx] = as_global(q)[(size_t)row_of(j) * K4 + k4];
    }
}

// The scores of one group, in two calls: scan16_group_wait, then scan16_group_mfma; scan16_group_scores is the pair.  A kernel
// that has a load of its own to send under the group's MFMAs (the masked kernel's next mask word) places it between the two.
//
// scan16_group_wait: the once-per-group wait for everything the wave has in flight -- the group's first PF chunks in the ring
// and whatever the last epilogue left; the chunk loop then starts from a clean state (see scanq_kernel) and waits counted,
// vmcnt(PF - 1), inside.
__device__ __forceinline__ void scan16_group_wait() {
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0) only
}
// scan16_group_mfma: acc += the group at gp (its first PF chunks in `ring`, arrived) times the tile's queries; on return `ring`
// holds the first PF chunks of the group at np, in flight (np == gp behind the last group: a live address, loaded and dropped),
// and gp = np.  qb = ldsQ + the lane's query slot.  K4 is a multiple of PF; at K4 == PF the chunk loop runs no block.
__device__ __forceinline__ void scan16_group_mfma(f32x16 &acc, f4 (&ring)[PF], gf4ptr &gp, gf4ptr np, const f4 *qb, int QTr, int K4) {
    const int NB = K4 / PF;
    // B (query) fragments run one chunk ahead of the MFMAs; the sched_barrier after every
    // chunk pins "consume ring[i] -> refill ring[i]" in program order, otherwise hipcc
    // clusters the eight refills at the end of the block and waits vmcnt(0) on them.
    f4 bcur = qb[0], bnxt;
    for (int tb = 0; tb < NB - 1; ++tb) {
#pragma unroll
        for (int i = 0; i < PF; ++i) {
            const int t = tb * PF + i;
            bnxt = qb[(t + 1) * QTr];
            const f4 av = ring[i];
            HAC_MFMA4(av, bcur)
            // refill AFTER the MFMAs that read ring[i]: the load can then reuse the register;
            // issued before them it gets a fresh one and hipcc copies it back at the loop
            // end behind vmcnt(7)...vmcnt(0) — a full drain every PF chunks
            ring[i] = gp[(t + PF) * 64];
            bcur = bnxt;
            __builtin_amdgcn_sched_barrier(0);
        }
    }
#pragma unroll
    for (int i = 0; i < PF; ++i) {
        const int t = (NB - 1) * PF + i;
        bnxt = qb[(i + 1 < PF ? t + 1 : 0) * QTr];
        const f4 av = ring[i];
        HAC_MFMA4(av, bcur)
        ring[i] = np[i * 64];  // next group's first chunks stay in flight across the epilogue
        bcur = bnxt;
        __builtin_amdgcn_sched_barrier(0);
    }
    gp = np;
}
__device__ __forceinline__ void scan16_group_scores(f32x16 &acc, f4 (&ring)[PF], gf4ptr &gp, gf4ptr np, const f4 *qb, int QTr, int K4) {
    scan16_group_wait();
    scan16_group_mfma(acc, ring, gp, np, qb, QTr, K4);
}

// Behind barrier (B) of a top-k kernel's round, when all appends of the round are visible: wave w looks at the candidate
// lists jj = w, w + SCAN_WAVES, ... of the tile.  A list above the high-water mark hw (= C - 64 * SCAN_WAVES >= k: a round
// appends at most 64 * SCAN_WAVES keys to a list) is sorted and cut to its best k, and its k-th score is offered to the chip
// (tglob = thr_glob + q0); every list's threshold takes the chip's, which other workgroups may have raised.
__device__ __forceinline__ void scan16_compact_round(u64 *cand, u32 *cnt, float *thr, u32 *tglob, int C, int k, u32 hw, int QTr, int w, int lane) {
    for (int jj = w; jj < QTr; jj += SCAN_WAVES) {
        const u32 n = cnt[jj];
        float t_new = -INFINITY;
        if (n > hw) {  // wave-uniform
            wave_sort_desc(cand + (size_t)jj * C, n, lane);
            t_new = ord2f((u32)(cand[(size_t)jj * C + k - 1] >> 32));
        }
        if (lane == 0) {
            float t_cur = thr[jj];
            if (n > hw) {
                cnt[jj] = k;
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
}

// End of a top-k kernel (behind a barrier): the tile's candidate lists go to the merge, wave w's as in the compaction round.
__device__ __forceinline__ void scan16_flush(const ScanArgs &a, u32 n_streams, int q0, int QTr, u64 *cand, const u32 *cnt, int C, int w, int lane) {
    for (int jj = w; jj < QTr; jj += SCAN_WAVES) flush_survivors(a, n_streams, q0 + jj, cand + (size_t)jj * C, cnt[jj], lane);
}
