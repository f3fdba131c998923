// gemm8.inc — the large-batch GEMM of the encoder: C = A[M,K] . W[N,K]^T with fused epilogues, 256x256x64 tiles,
// 8 waves in two groups that alternate between a memory segment and a matrix segment ("ping-pong"): while the four
// waves of one group issue their 16 MFMAs of a phase, the other four read fragments from LDS and issue the LDS-DMA
// of a later k-tile.  Included by encoder.hip inside namespace hac { namespace {.
//
// Structure (cdna_hip_programming.md §5, "The 256^2 8-phase template", rebuilt here from its description and reshaped):
//   * LDS = half-tile slots of 16 KiB in two rings: activations three k-tiles (6 slots at 0), weights two (4 slots at
//     96 KiB), 160 KiB in all.  A half-tile is 128 rows x 64 k of bf16, 128-byte rows, 16-byte chunk c of row r at
//     r*128 + ((c ^ ((r >> 1) & 7)) << 4) (conflict-free ds_read_b128); filled by LDS-DMA in 1-KiB pieces with the swizzle
//     applied to the per-lane SOURCE address, the destination being lane-linear.
//   * wave (wr, wc) of the 2 x 4 grid owns rows {i*128 + wr*64 .. +64 : i = 0,1} and columns {j*128 + wc*32 .. +32 :
//     j = 0,1} of the tile, so that quadrant (i, j) of its accumulators needs exactly half-tiles A_i and W_j.
//     A k-tile is two phases of 32 MFMAs: phase 1 reads W_0, W_1, A_0 (16 x ds_read_b128) and computes the upper row half
//     Q(0,0), Q(0,1); phase 2 reads A_1 INTO THE SAME REGISTERS (8 reads) and computes Q(1,0), Q(1,1).  Each phase: DMA
//     pieces + reads + lgkmcnt(0) | s_barrier | 32 x v_mfma_f32_16x16x32_bf16 | s_barrier; inside a tile's k-loop group 1
//     runs one barrier behind group 0.  (The template's four 16-MFMA phases per k-tile measured 513 cycles per barrier
//     interval against 256 of matrix work: in-kernel stamps showed ~190 cycles of DMA issue + addressing per half-tile and
//     ~100 of barrier / wait overhead per phase; two phases per k-tile halve the barriers per MFMA.)
//   * the two wave groups stage different operands -- group 0 the activation half-tiles (HBM stream), group 1 the weight
//     half-tiles (L2 hits) -- N1 of a k-tile's eight pieces per wave in phase 1 and 8 - N1 in phase 2 (the phase with fewer
//     fragment reads takes more of the DMA issue).  Each wave's in-order vmcnt queue holds ONE kind of load, so a wait for
//     the next weights does not wait for every older activation load.  (Measured on the earlier form, whose phases read
//     20 + 4 fragments and in which every wave staged both operands: a k-tile took ~3200 cycles against 2 x 2 x 580 of
//     matrix work per SIMD, because the phase that reads 20 fragments (~400 cycles: the four waves of a group saturate the
//     LDS pipe) and issues 4 DMA pieces (~95 cycles each) lasted ~820 cycles beside the partner's 580 of MFMAs, while the
//     other loading phase was done in 540.  16 + 8 reads balance the two, and need 32 VGPRs fewer.  In the 1000 x 512
//     forward, two boxes: FFN-down (K = 3072) -1 .. -3.4 %, the K = 768 GEMMs inside the run-to-run spread, the layer stack
//     93.4 - 94.9 ms against 95.3 - 96.7.)
//   * the DMA stream never drains inside the loop.  At the start of k-tile T activations are issued up to T+1 and land
//     four barrier intervals after their last piece; weights up to T+1 (the last N1 pieces of T+1 go out in phase 1 of T),
//     waited for in phase 2 of T.  A slot is restaged only after both groups retired their reads of it (lgkmcnt(0) BEFORE
//     the barrier) at least one barrier earlier.  The activation rows, which stream from HBM, run further ahead of their
//     use than the weight rows (measured: the k-loop with every DMA redirected to an L2-resident tile was 12-17 % faster).
//     The stream continues across output tiles (persistent workgroups, XCD-aware tile runs), so neither the first load of a
//     tile nor the epilogue's stores stall the matrix pipe.
//   * QKV and FFN-up (EPI != EPI8_RESID) run ONE phase per k-tile and group instead of the two described above: DMA pieces + 16 reads +
//     lgkmcnt(0) | s_barrier | 64 MFMAs with the eight A_1 reads woven in (into the registers A_0 was in: no register more) | s_barrier
//     -- two barrier intervals per k-tile, not four.  There group 0 stages the WEIGHTS and group 1 the ACTIVATIONS: each operand is staged
//     by the group that reads it LAST, so that group's own program order, not a barrier, stands between its last read of a slot and the
//     restage, and a whole k-tile goes out in the one loading part that follows.  Barriers b1, b2, ... of a tile, interval I_n between
//     b_n and b_n+1; L(T) = loading part, M(T) = matrix part of k-tile T; group 0: L(T) in I_2T, M(T) in I_2T+1; group 1 one later:
//         k-tile T   group 0 reads in   group 1 reads in   slot free from   restaged by, in            with
//         W_0, W_1   I_2T               I_2T+1             I_2T+2           group 0, L(T+1) = I_2T+2   W(T+2)
//         A_0        I_2T               I_2T+1             I_2T+2           group 1, L(T+1) = I_2T+3   A_0(T+3)
//         A_1        I_2T+1 (woven)     I_2T+2 (woven)     I_2T+3           group 1, L(T+1) = I_2T+3   A_1(T+3)
//       (every read retired, lgkmcnt(0), before the barrier that closes its interval).  Look-ahead, always the staging group's own vmcnt
//       in front of the barrier behind which the first reader starts:
//         W(T+1)   issued at the head of group 0's L(T), I_2T     vmcnt(0) at the END of group 0's M(T), I_2T+1; first read I_2T+2:
//                  ~1.7 long intervals, ~2200 cycles (two-phase form: ~1500)
//         A(T+2)   issued at the head of group 1's L(T), I_2T+1   vmcnt(8) -- all but L(T+1)'s own pieces -- at the end of group 1's
//                  L(T+1), I_2T+3; first read (A_0, by group 0) I_2T+4: ~2.7 long intervals, ~3500 cycles (two-phase form: ~3000)
//     Seams, prologue, stream end: every tile's k-loop starts from A and W k-tiles 0 and 1 landed (prologue: 16 pieces per wave).  Group 1
//     issues A(T+2) in every L(T) (T = KT-2, KT-1: the next tile's k-tiles 0, 1); group 0 issues W(T+1) in L(T) for T >= 1 and the next
//     tile's k-tile 1 at the seam, where both groups drain BEFORE the epilogue's stores.  A tile's first k-tile has no vmcnt wait (it
//     would wait for the previous epilogue's stores).  A loading part that issued nothing (h_left) waits vmcnt(0).
//     Measured: a steady QKV k-tile 2460 - 2700 cycles against 3100; 512000 rows: QKV 1.72 -> 1.63 ms, FFN-up 2.38 -> 2.28 ms.  With the
//     two-phase roles (weights landed inside the loading part that issued them) group 1 waited 370 - 480 cycles per k-tile: +1 %; weight
//     pieces at the head of the matrix part cost 100 - 120 cycles each there: slower than two phases (LABNOTES, "gemm8: one phase").
//   * accumulators are held TRANSPOSED (MFMA A operand = W rows, B operand = activation rows): lane (m = lane & 15,
//     g = lane >> 4) owns, for token row m, output features 4g .. 4g+3 of every 16-feature tile -- four consecutive
//     fp32 = one 16-byte access to the residual stream, and after one v_permlane16_swap per packed register eight
//     consecutive bf16 = one 16-byte store.  No LDS round trip, no patch buffers.  The V projection, whose output layout
//     is token-contiguous, transposes 4x4 blocks inside each quad of lanes (DPP) and stores 8 bytes per lane.
//   * LayerNorm is folded into the consumer: the producer (RESID epilogue) writes the un-normalized row y once, in bf16
//     (it is the next GEMM's A operand and the next residual), and per-row partial sums of the fp32 values; the consumer
//     multiplies by W' = W.diag(gamma) and finishes out = rstd[m] * (acc - mean[m] * wsum[n]) + cvec[n], wsum = W'.1,
//     cvec = bias + W.beta.  No LayerNorm pass over HBM remains between the GEMMs, and the residual stream costs 2 + 2
//     bytes per element and GEMM instead of 4 + 4 + 2 (measured: the epilogues cost time in proportion to their bytes).

enum { EPI8_QKV = 0, EPI8_RESID = 2, EPI8_GELU = 3 };
#ifndef G8_N1
#define G8_N1 4   // DMA pieces (of a k-tile's 8 per wave) issued in the phase that reads 16 fragments; the 8-read phase takes the rest
#endif

struct Gemm8Args {
    const bf16 *A;           // [Mp][K] row-major, Mp a multiple of 256
    const bf16 *W;           // [N][K] row-major (LayerNorm gamma already folded in where astats is used)
    int N, K;                // multiples of 256 / 64
    int n_groups;            // 1, 2 or 4 (must divide N / 256 - n_tile0): column groups the XCDs split W into
    int n_tile0;             // first column tile computed (the last layer's QKV skips Q's three: only the <s> rows need it)
    const int *total_rows;   // device: rows in use; tiles starting beyond it are skipped
    // QKV / GELU: folded LayerNorm of the A rows
    const float2 *astats;    // [Mp] (mean, rstd)
    const float *wsum;       // [N]
    const float *cvec;       // [N]   (RESID: the bias)
    bf16 *q, *k, *v16;       // QKV (N = 2304: q | k | v): q, k [Mp][768]; v16 [Mp/16][768][16]
    // RESID: y = acc + cvec[n] + r,  r = resid or, with rstats, (resid - mean) * rstd * rgamma + rbeta.  The residual stream
    // lives in bf16 between the GEMMs (row statistics are taken from the fp32 sums before the one rounding).
    const bf16 *resid;       // [Mp][N]
    const float2 *rstats;
    const float *rgamma, *rbeta;
    bf16 *yb;                // [Mp][N] y, the next GEMM's A operand and the next residual
    float2 *part;            // [Mp][N/64] per-row (sum, sum of squares) over the 64 columns one wave owns (tile n0/256, wave column wc)
    bf16 *h;                 // GELU: [Mp][N]
    unsigned long long *clk; // GELU only, may be null: [4] = (s_memtime, s_memrealtime) at workgroup 0's first and last instruction
    int stagger;             // start delay in ~1-us sleeps per phase step (0 = none): see gemm8_kernel, "phases"
    int stagger_mode;        // which workgroups share a phase: 0 = xcd & 3, 1 = slot & 3, 2 = xcd, 3 = slot & 7
};

__device__ __forceinline__ void glds16(const bf16 *src, unsigned char *dst) {
    typedef const __attribute__((address_space(1))) void *gvp;
    typedef __attribute__((address_space(3))) void *lvp;
    __builtin_amdgcn_global_load_lds((gvp)src, (lvp)dst, 16, 0, 0);
}
// two packed-bf16 registers of feature tiles nt = 0 (a) and nt = 1 (b): afterwards lane group g holds eight consecutive
// features starting at 8 * ((g & 1) * 2 + (g >> 1)) of the 32-column band
__device__ __forceinline__ void swap16(unsigned &a, unsigned &b) {
    const auto r = __builtin_amdgcn_permlane16_swap(a, b, false, false);
    a = r[0];
    b = r[1];
}
// 4x4 transpose across the four lanes of a quad (p = lane & 3): afterwards component t of lane p is what component p of
// lane t was.  Two butterfly stages of DPP quad permutes.
__device__ __forceinline__ void quad_transpose4(f4v &v, int p) {
    int x0 = __float_as_int(v.x), x1 = __float_as_int(v.y), x2 = __float_as_int(v.z), x3 = __float_as_int(v.w);
    {   // lanes p and p^1 exchange: even p sends component 1 / 3 and receives into them, odd p component 0 / 2
        const bool odd = p & 1;
        const int sa = odd ? x0 : x1, sb = odd ? x2 : x3;
        const int ra = __builtin_amdgcn_update_dpp(0, sa, 0xB1, 0xF, 0xF, false);   // quad_perm [1,0,3,2]
        const int rb = __builtin_amdgcn_update_dpp(0, sb, 0xB1, 0xF, 0xF, false);
        x0 = odd ? ra : x0;
        x1 = odd ? x1 : ra;
        x2 = odd ? rb : x2;
        x3 = odd ? x3 : rb;
    }
    {   // lanes p and p^2: p < 2 sends components 2, 3, p >= 2 components 0, 1
        const bool hi = p & 2;
        const int sa = hi ? x0 : x2, sb = hi ? x1 : x3;
        const int ra = __builtin_amdgcn_update_dpp(0, sa, 0x4E, 0xF, 0xF, false);   // quad_perm [2,3,0,1]
        const int rb = __builtin_amdgcn_update_dpp(0, sb, 0x4E, 0xF, 0xF, false);
        x0 = hi ? ra : x0;
        x2 = hi ? x2 : ra;
        x1 = hi ? rb : x1;
        x3 = hi ? x3 : rb;
    }
    v.x = __int_as_float(x0);
    v.y = __int_as_float(x1);
    v.z = __int_as_float(x2);
    v.w = __int_as_float(x3);
}

// Line-shaped epilogue accesses.  After swap16 a lane (token row m16, lane group kg) holds, for each of the wave's two
// 32-column bands j, one 16-byte chunk of ITS row: an access instruction over (j fixed) would touch 16 rows x 64 bytes.
// xchg8 trades chunks between lanes m16 and m16 ^ 8 (DPP row_ror:8): afterwards (a, b) are the chunks of band m16 >> 3 of
// rows (m16 & 7) and 8 + (m16 & 7) -- instruction "a" covers rows 0..7 of the 16-row block, "b" rows 8..15, each row's whole
// 128-byte line (wc*64 .. +64 columns).  The exchange is its own inverse: applied to what two such loads returned it gives
// (band 0, band 1) of the lane's own row back.  Measured with the addresses alone rewired (wrong data, same bytes): the
// RESID epilogue 35 k -> 30 k cycles per tile.
__device__ __forceinline__ void xchg8(uint4 &a, uint4 &b, bool lo) {
    unsigned *pa = reinterpret_cast<unsigned *>(&a), *pb = reinterpret_cast<unsigned *>(&b);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const unsigned send = lo ? pb[i] : pa[i];
        const unsigned recv = (unsigned)__builtin_amdgcn_update_dpp(0, (int)send, 0x128, 0xF, 0xF, false);   // row_ror:8
        pa[i] = lo ? pa[i] : recv;
        pb[i] = lo ? recv : pb[i];
    }
}

// The epilogues' output stores.  NT: non-temporal -- the q / k / v and h streams (2.3 and 3.1 GB per launch at 512000 rows, more
// than those kernels read) are consumed by a LATER kernel; written with the default policy they push the weight and activation
// lines the k-loop is about to re-read out of the 4-MB L2 (tools/probes/gemm8_stagger_probe.hip, G8_BASE_ONLY: QKV -2.6 %, FFN-up
// -3.5 %; inside the 1000 x 512 forward -1.0 ms of 92.5).  The residual stream's stores stay temporal: RESID with NT measured
// +1.5 % (out-proj) / +1.8 % (FFN-down); its residual LOADS with the bit: nothing.  The activation DMA with the non-temporal
// bit (rows are read once per XCD): -6 % everywhere, not used.  (gemm8_kernel takes the policy as its template parameter NT.)
typedef unsigned g8_u4 __attribute__((ext_vector_type(4)));
typedef unsigned g8_u2 __attribute__((ext_vector_type(2)));
template <bool NT> __device__ __forceinline__ void g8_store16(void *p, uint4 v) {
    if constexpr (NT) __builtin_nontemporal_store(g8_u4{v.x, v.y, v.z, v.w}, reinterpret_cast<g8_u4 *>(p));
    else *reinterpret_cast<uint4 *>(p) = v;
}
template <bool NT> __device__ __forceinline__ void g8_store8(void *p, uint2 v) {
    if constexpr (NT) __builtin_nontemporal_store(g8_u2{v.x, v.y}, reinterpret_cast<g8_u2 *>(p));
    else *reinterpret_cast<uint2 *>(p) = v;
}

__device__ __forceinline__ unsigned pack_bf16(float lo, float hi) {
    typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
    bf16x2_t v;
    v.x = (bf16)lo;
    v.y = (bf16)hi;
    return __builtin_bit_cast(unsigned, v);
}

// erf GELU as x * G(x), G(x) = 0.5 + z Ph(z^2), z = clamp(x / sqrt 2, -3, 3), Ph = half of a degree-7 fit of erf(z)/z
// constrained to erf(3) = 1 (the clamped tails give exactly x and 0): |GELU error| <= 8.2e-5 absolute, the accuracy of the
// classic kernels' degree-8 form, in 3 packed multiplies + 8 packed fma + 2 med3 per PAIR of elements.
__device__ __forceinline__ f2v gelu8_2(f2v x) {
    f2v z = x * 0.70710678118654752f;
    z.x = __builtin_amdgcn_fmed3f(z.x, -3.0f, 3.0f);
    z.y = __builtin_amdgcn_fmed3f(z.y, -3.0f, 3.0f);
    const f2v u = z * z;
    f2v p = u * (-1.546677965e-07f) + 6.9032217e-06f;
    p = p * u + (-0.0001336812065f);
    p = p * u + 0.001487465865f;
    p = p * u + (-0.0106578986f);
    p = p * u + 0.0524059485f;
    p = p * u + (-0.1851637965f);
    p = p * u + 0.56346134f;
    return x * (z * p + 0.5f);
}

// NT: the output stores are non-temporal (see g8_store16); the encoder sets it for QKV and GELU.
template <int EPI, bool NT>
__global__ __launch_bounds__(512, 2) void gemm8_kernel(Gemm8Args g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = w >> 2, wc = w & 3;
    if constexpr (EPI == EPI8_GELU) {   // the launch's shader clock (hac_encoder_last_clock): both counters, stored at once
        if (g.clk && blockIdx.x == 0 && tid == 0) {
            g.clk[0] = __builtin_amdgcn_s_memtime();
            g.clk[1] = __builtin_amdgcn_s_memrealtime();
        }
    }
    const int K = g.K, KT = K >> 6, nx = (g.N >> 8) - g.n_tile0;
    // XCD-aware tile runs: workgroups are dealt round-robin over the 8 XCDs.  XCD x owns column group x % n_groups (nx /
    // n_groups column tiles: that part of W stays in its L2) and the (x / n_groups)-th share of the row tiles; inside the
    // run consecutive tiles share their A rows, and the XCD's workgroups take the tiles round-robin.
    const int NG = g.n_groups, nxg = nx / NG, NP = 8 / NG;
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, per_xcd = (gridDim.x + 7 - xcd) >> 3;
    const int mt_all = (*g.total_rows + 255) >> 8;
    const int mt_lo = (int)((long)mt_all * (xcd / NG) / NP), mt_hi = (int)((long)mt_all * (xcd / NG + 1) / NP);
    const int n_base = g.n_tile0 + (xcd % NG) * nxg;
    const int run_lo = 0, run_hi = (mt_hi - mt_lo) * nxg;     // local tile index l -> (mt_lo + l / nxg, n_base + l % nxg)
    const int tile0 = run_lo + slot;
    if (tile0 >= run_hi) return;
    const int my_tiles = (run_hi - tile0 + per_xcd - 1) / per_xcd;
    // ---- the DMA stream: this wave's 1-KiB pieces of ONE operand (`so` below; RESID: group 0 A, group 1 W) in the order k-tile, half, piece,
    // over all the workgroup's output tiles.  A half-tile (128 rows x 128 B) is 16 pieces of 8 rows; wave quarter wq = w & 3 of
    // the staging group moves rows wq*32 .. +32 as pieces p = 0..3 (rows +8p; even p: swizzle f(row) = lane >> 4, odd p:
    // 4 + (lane >> 4)).
    // The W half-tiles are filled with PERMUTED rows: LDS row r of half j holds output column (r >> 5) * 64 + j * 32 + (r & 31)
    // of the tile, so that wave column wc (which reads LDS rows wc*32 .. +32 of both halves) owns the 64 CONTIGUOUS columns
    // wc*64 .. +64 -- one 128-byte line per output row, which the epilogues read and write whole (see there).  LDS rows
    // wq*32 .. +32 of W half j are therefore W rows wq*64 + j*32 .. +32.
    const int srow = lane >> 3;
    const int sch0 = (lane & 7) ^ (srow >> 1);
    // the lane's swizzled 16-byte chunk in an even / odd piece, in elements.  (Formed here, before the tile pointers: where the
    // optimizer first meets these values decides the instruction schedule of every instantiation -- checked by disassembly.)
    const int chE = sch0 * 8, chO = (sch0 ^ 4) * 8;
    int s_tile = tile0, s_kt = 0;
    const bf16 *s_A = g.A + (size_t)((mt_lo + s_tile / nxg) << 8) * K, *s_W = g.W + (size_t)((n_base + s_tile % nxg) << 8) * K;
    const int wq = w & 3;
    // the operand this wave's group stages: 0 = activations, 1 = weights.  RESID: group 0 the activations.  QKV / GELU, whose groups
    // run ONE phase per k-tile: group 0 the weights -- each operand is staged by the group that is the LAST to read it (see the k-loop)
    const int so = EPI == EPI8_RESID ? wr : wr ^ 1;
    // 32-bit lane offsets on top of a workgroup-uniform base: the DMA takes its address as SGPR pair + one VGPR
    const unsigned lsrcE = (unsigned)(((so ? wq * 64 : wq * 32) + srow) * K + chE);
    const unsigned lsrcO = (unsigned)(((so ? wq * 64 : wq * 32) + 8 + srow) * K + chO);
    const int ring_base = (so ? 98304 : 0) + wq * 4096, ring_slots = so ? 4 : 6;
    int h_half = 0, h_slot = 0, h_p = 0;
    const bf16 *h_base = so ? s_W : s_A;
    long h_left = (long)my_tiles * KT * 8;
    constexpr int N1 = G8_N1, N2 = 8 - N1;             // pieces per wave issued in phase 1 / phase 2 of a k-tile
    auto issue_piece = [&]() __attribute__((always_inline)) {
        const bf16 *src = h_base + (size_t)(h_half * (so ? 32 : 128) + (h_p >> 1) * 16) * K + s_kt * 64;
        unsigned char *dst = smem + ring_base + (h_slot << 14) + h_p * 1024;
        glds16(src + ((h_p & 1) ? lsrcO : lsrcE), dst);
        if (++h_p == 4) {
            h_p = 0;
            h_slot = h_slot + 1 == ring_slots ? 0 : h_slot + 1;
            if (++h_half == 2) {
                h_half = 0;
                if (++s_kt == KT) {
                    s_kt = 0;
                    s_tile += per_xcd;
                    h_base = so ? g.W + (size_t)((n_base + s_tile % nxg) << 8) * K : g.A + (size_t)((mt_lo + s_tile / nxg) << 8) * K;
                }
            }
        }
    };
    // n pieces, or none once the stream has ended (it ends on a k-tile boundary); group-uniform
    auto issue_pieces = [&](auto ntag) __attribute__((always_inline)) -> bool {
        constexpr int n = decltype(ntag)::value;
        if (h_left <= 0) return false;
        h_left -= n;
#pragma unroll
        for (int i = 0; i < n; ++i) issue_piece();
        return true;
    };
    constexpr std::integral_constant<int, 16> n16tag{};
    constexpr std::integral_constant<int, 8> n8ktag{};

    // ---- fragment addresses inside a k-tile buffer: slots A0 | A1 | W0 | W1
    const int m16 = lane & 15, kg = lane >> 4, sw = (m16 >> 1) & 7;
    const int c0 = ((kg ^ sw) << 4), c1 = (((4 + kg) ^ sw) << 4);            // k-steps 0 and 1 of the lane's 16-byte chunk
    const int a_row = (wr * 64 + m16) * 128, w_row = (wc * 32 + m16) * 128;   // + mt*2048 / nt*2048

#ifdef G8_STAMP
    unsigned long long stamps[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long est[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // the LDS-landed RESID epilogue of tile 2, step by step
#define G8_T(i, cond) if (cond) stamps[i] = __builtin_amdgcn_s_memtime()
#define G8_E(i) if (seq == 2) est[i] = __builtin_amdgcn_s_memtime()
#else
#define G8_E(i)
#define G8_T(i, cond)
#endif
#ifdef G8_STAMP2   // phase-level stamps of one steady-state k-tile (tile 3, k-tile 6): where a barrier interval goes
    unsigned long long ph[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#define G8_P(i) if (seq == 3 && kt == 6) ph[i] = __builtin_amdgcn_s_memtime()
// the one-phase loop (QKV / GELU) has no second loading part: between its two halves of 32 MFMAs, in every stamp of that part
#define G8_PM() if (seq == 3 && kt == 6) ph[5] = ph[6] = ph[13] = ph[7] = ph[8] = ph[9] = __builtin_amdgcn_s_memtime()
#else
#define G8_P(i)
#define G8_PM()
#endif
    constexpr bool RL = EPI == EPI8_RESID;   // the RESID epilogue lands its inputs in LDS (see the epilogue)
    f32x4 acc[2][2][4][2];   // [i][j][mt][nt]
    bf16x8 wf0[2][2], wf1[2][2], af0[4][2];   // [nt or mt][ks]

    // the state every tile's k-loop starts from: activation and weight k-tiles 0 and 1 staged and landed
    issue_pieces(n16tag);
    if (g.stagger) {   // phases: workgroups that start together reach their epilogues together (see Gemm8Args::stagger)
        const int ph = g.stagger_mode == 0 ? (xcd & 3) : g.stagger_mode == 1 ? (slot & 3) : g.stagger_mode == 2 ? xcd : (slot & 7);
        for (int i = ph * g.stagger; i > 0; --i) __builtin_amdgcn_s_sleep(32);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();

    int a_cur = 0, w_cur = 0;                          // ring positions of the k-tile being read
    for (int seq = 0; seq < my_tiles; ++seq) {
        const int tile = tile0 + seq * per_xcd;
        const int m0 = (mt_lo + tile / nxg) << 8, n0 = (n_base + tile % nxg) << 8;
        // RL (the RESID epilogue that lands its inputs in LDS, see the epilogue): per-wave regions and DMA sources of this tile
        unsigned char *R1 = smem, *R2 = smem, *R3 = smem;
        const size_t rl_tb = (size_t)m0 * H + n0;
        // (the lane-dependent part of every source address is formed AT the issue point -- `ln` is opaque to the optimizer --: hoisted
        // to the tile's start these 64-bit per-lane pointers were six register pairs live across the k-loop, i.e. spills)
        auto rl_issue_sb = [&](int i, int mt, unsigned char *dst) __attribute__((always_inline)) {
            // sub-band (i, mt): the wave's rows i*128 + wr*64 + mt*16 .. +16, its 64 columns; DMA lane l = (nt = l >> 5, a = (l >> 4) & 1,
            // m = l & 15) brings the eight features nt*16 + 8a .. +8 of row m of band j (one instruction per band)
            int ln = lane;
            asm volatile("" : "+v"(ln));
            const unsigned lo = (unsigned)((ln & 15) * H + (ln >> 5) * 16 + ((ln >> 4) & 1) * 8);
#if defined(G8_RL_ABL) && (G8_RL_ABL & 2)   // timing only: every sub-band from one cache-resident place
            const bf16 *src = g.resid + (size_t)(wr * 64 + i * 128 + mt * 16) * H + wc * 64 + lo;
#else
            const bf16 *src = g.resid + (rl_tb + (size_t)(wr * 64 + i * 128 + mt * 16) * H + wc * 64) + lo;
#endif
            glds16(src, dst);
            glds16(src + 32, dst + 1024);
        };
        auto rl_issue_cols = [&](unsigned char *dst) __attribute__((always_inline)) {
            int ln = lane;
            asm volatile("" : "+v"(ln));
            // (mean, rstd) of the wave's 2 x 64 rows: lane l brings rows 2*(l & 31), +1 of band l >> 5.  (Rows that are final -- layer
            // 0's embedding rows -- come with identity statistics and gamma = 1, beta = 0 from the host: no branch here.)
            const unsigned so = (unsigned)((ln >> 5) * 128 + 2 * (ln & 31));
            glds16(reinterpret_cast<const bf16 *>(g.rstats + ((size_t)m0 + wr * 64) + so), dst);
            // bias | gamma | beta of the wave's 64 columns: lanes 0..15 / 16..31 / 32..47 (48..63: bias again, unused)
            const int sel = (ln >> 4) & 3;
            // (the three pointers as VALUES in scalar registers: left to itself hipcc selects between the kernel ARGUMENTS' addresses
            // and loads the chosen one with a vector load -- a vmcnt(0) in the middle of the DMA stream)
            const float *pc = g.cvec, *pg = g.rgamma, *pb = g.rbeta;
            asm volatile("" : "+s"(pc), "+s"(pg), "+s"(pb));
            const float *vb = pc;
            vb = sel == 1 ? pg : vb;
            vb = sel == 2 ? pb : vb;
            glds16(reinterpret_cast<const bf16 *>(vb + (n0 + wc * 64) + 4 * (ln & 15)), dst + 1024);
        };
        // Inside a tile's k-loop group 1 runs one barrier behind group 0 (one group computes while the other reads and
        // stages); around the epilogue the groups are aligned again, or their epilogues (long: HBM latency, store issue)
        // would run one after the other instead of side by side.
        G8_T(2, seq == 3);                           // the epilogue of tile 2 has been issued
        if (wr == 1) __builtin_amdgcn_s_barrier();
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[i][j][mt][nt][e] = 0.f;

        for (int kt = 0; kt < KT; ++kt) {
            G8_P(0);
            const unsigned char *kbA = smem + a_cur * 32768, *kbW = smem + 98304 + w_cur * 32768;   // A_0 | A_1, W_0 | W_1
            if constexpr (!RL) {
                // ================ QKV / GELU: ONE phase per k-tile and group (two barrier intervals; tables in the header)
                // ---------------- loading part: DMA pieces, then W_0, W_1, A_0 (the partner group is in its 64 MFMAs)
                // Group 0: weight k-tile T+1 (slots of T-1: group 1, the last to read them, retired those reads before the barrier
                // that closed the previous interval); a tile's first k-tile finds k-tile 1 staged.  Group 1: activation k-tile T+2
                // (slots of T-1: its A_1 half was read last by this group's own matrix part, which ended at the barrier above).
                // The pieces go out BEFORE the fragment reads (a DMA instruction behind ds_reads of its own wave: ~100 cycles each).
                const bool staged = (wr || kt) && issue_pieces(n8ktag);
                __builtin_amdgcn_sched_barrier(0);
                G8_P(12);
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    wf0[nt][0] = *reinterpret_cast<const bf16x8 *>(kbW + w_row + nt * 2048 + c0);
                    wf0[nt][1] = *reinterpret_cast<const bf16x8 *>(kbW + w_row + nt * 2048 + c1);
                    wf1[nt][0] = *reinterpret_cast<const bf16x8 *>(kbW + 16384 + w_row + nt * 2048 + c0);
                    wf1[nt][1] = *reinterpret_cast<const bf16x8 *>(kbW + 16384 + w_row + nt * 2048 + c1);
                }
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) {
                    af0[mt][0] = *reinterpret_cast<const bf16x8 *>(kbA + a_row + mt * 2048 + c0);
                    af0[mt][1] = *reinterpret_cast<const bf16x8 *>(kbA + a_row + mt * 2048 + c1);
                }
                __builtin_amdgcn_sched_barrier(0);
                G8_P(1);
                // Group 1: landed before this barrier, for BOTH groups' reads behind it, is everything older than this part's pieces,
                // i.e. activation k-tile T+1, whose A_0 group 0 reads in the next interval (issued two intervals ago).  A tile's
                // first k-tile waits for nothing: what it needs was drained before the previous epilogue, and a counted wait would
                // also wait for that epilogue's stores (one in-order queue per wave).  Group 0 waits at the END of its matrix part.
                G8_P(2);
                if (wr && kt) {
                    if (staged) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
                    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                }
                // the reads are retired BEFORE the barrier: the other group may restage the W and A_0 slots right after it
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                G8_P(3);
                __builtin_amdgcn_s_barrier();
                G8_P(4);
                G8_T(3 + (kt < 3 ? kt : 3), seq == 3 && kt < 4);   // first barrier of k-tiles 0..3 of tile 3
                __builtin_amdgcn_sched_barrier(0);
                // ---------------- matrix part: 64 MFMAs between two barriers
                __builtin_amdgcn_s_setprio(1);
                // Q(0,0), Q(0,1), then Q(1,0), Q(1,1), each in the order (ks, mt, nt).  The read of A_1[mt][ks] goes into af0[mt][ks]
                // behind the last of the four MFMAs that use that register -- except the last two, A_1[2][1] and A_1[3][1], which go
                // out behind the first two MFMA groups of the lower half.  Why: hipcc cannot count LDS reads past an LDS-DMA
                // instruction whose vmcnt it has not seen reach zero (it books the DMA on lgkmcnt too, and this loop never drains
                // vmcnt), so the wait it places before the first use of a fragment is lgkmcnt(0), whatever was asked for.  This
                // order puts eight MFMAs (>= 128 cycles) between the youngest read and each of the two places where it waits:
                // MFMA 33 (A_1[.][0], and [0..1][1]) and MFMA 57 ([2..3][1]).
                auto read_a1 = [&](auto mttag, auto kstag) __attribute__((always_inline)) {
                    constexpr int mt = decltype(mttag)::value, ks = decltype(kstag)::value;
                    __builtin_amdgcn_sched_barrier(0);
                    af0[mt][ks] = *reinterpret_cast<const bf16x8 *>(kbA + 16384 + a_row + mt * 2048 + (ks ? c1 : c0));
                    __builtin_amdgcn_sched_barrier(0);
                };
                constexpr std::integral_constant<int, 0> i0{};
                constexpr std::integral_constant<int, 1> i1{};
                constexpr std::integral_constant<int, 2> i2{};
                constexpr std::integral_constant<int, 3> i3{};
                auto mfma4 = [&](auto itag, auto mttag, auto kstag) __attribute__((always_inline)) {
                    constexpr int i = decltype(itag)::value, mt = decltype(mttag)::value, ks = decltype(kstag)::value;
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt) {
                        acc[i][0][mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf0[nt][ks], af0[mt][ks], acc[i][0][mt][nt], 0, 0, 0);
                        acc[i][1][mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf1[nt][ks], af0[mt][ks], acc[i][1][mt][nt], 0, 0, 0);
                    }
                };
                mfma4(i0, i0, i0), read_a1(i0, i0);
                mfma4(i0, i1, i0), read_a1(i1, i0);
                mfma4(i0, i2, i0), read_a1(i2, i0);
                mfma4(i0, i3, i0), read_a1(i3, i0);
                mfma4(i0, i0, i1), read_a1(i0, i1);
                mfma4(i0, i1, i1), read_a1(i1, i1);
                mfma4(i0, i2, i1);
                mfma4(i0, i3, i1);
                __builtin_amdgcn_sched_barrier(0);
                G8_PM();
                mfma4(i1, i0, i0), read_a1(i2, i1);
                mfma4(i1, i1, i0), read_a1(i3, i1);
                mfma4(i1, i2, i0);
                mfma4(i1, i3, i0);
                __builtin_amdgcn_sched_barrier(0);
                mfma4(i1, i0, i1);
                mfma4(i1, i1, i1);
                mfma4(i1, i2, i1);
                mfma4(i1, i3, i1);
                __builtin_amdgcn_s_setprio(0);
                G8_P(10);
                // Group 0: weight k-tile T+1, issued in this k-tile's loading part a whole matrix part ago, has landed before the
                // barrier behind which group 0 itself is the first to read it (a tile's first k-tile: drained before the epilogue).
                if (wr == 0 && kt) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                // the A_1 reads are retired BEFORE the closing barrier: group 1 restages that half-slot right behind its own
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                G8_P(11);
                a_cur = a_cur == 2 ? 0 : a_cur + 1;
                w_cur ^= 1;
                continue;
            }
            // ================ RESID: two phases of 32 MFMAs per k-tile and group (four barrier intervals)
            // ---------------- phase 1: W_0, W_1, A_0 -> Q(0,0), Q(0,1)
            // Group 0 stages the first N1 pieces of activation k-tile T+2 (slots of T-1: every read of it retired two barriers
            // ago).  Group 1: the last N1 pieces of weight k-tile T+1 -- a tile's first k-tile finds them staged (issued and
            // drained before the previous epilogue, see the end of the k-loop).
            // The pieces go out BEFORE the phase's fragment reads: stamps showed a DMA instruction issued behind ds_reads of
            // its own wave costing ~100 cycles (4 pieces behind 20 reads: 390 cycles on top of the reads' 370) and ~200 when
            // pieces and reads alternate -- it appears to wait for the wave's LDS queue -- against ~60 among MFMAs.
            // RL (RESID, LDS-landed residual): the LAST k-tile of a tile does not stage the next tile's k-tile 1 -- its slots are
            // where the epilogue lands the residual; those 8 pieces per wave go out from inside the epilogue instead
            const bool lastk = RL && kt == KT - 1;
            const bool live1 = (wr == 0 || kt) && h_left > 0 && !(lastk && wr == 0);
            if (live1) {
                h_left -= N1;
#pragma unroll
                for (int i = 0; i < N1; ++i) issue_piece();
            }
            if constexpr (RL) {
                if (lastk) {   // R1: the slot the activation k-tile T+2 would have gone to (every read of it retired two barriers ago)
                    R1 = smem + (a_cur == 0 ? 2 : a_cur - 1) * 32768 + w * 4096;
                    R3 = smem + a_cur * 32768 + w * 4096;
                    R2 = smem + 98304 + w_cur * 32768 + w * 4096;
                    rl_issue_cols(R1);
                    rl_issue_sb(0, 0, R1 + 2048);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            G8_P(12);
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                wf0[nt][0] = *reinterpret_cast<const bf16x8 *>(kbW + w_row + nt * 2048 + c0);
                wf0[nt][1] = *reinterpret_cast<const bf16x8 *>(kbW + w_row + nt * 2048 + c1);
                wf1[nt][0] = *reinterpret_cast<const bf16x8 *>(kbW + 16384 + w_row + nt * 2048 + c0);
                wf1[nt][1] = *reinterpret_cast<const bf16x8 *>(kbW + 16384 + w_row + nt * 2048 + c1);
            }
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                af0[mt][0] = *reinterpret_cast<const bf16x8 *>(kbA + a_row + mt * 2048 + c0);
                af0[mt][1] = *reinterpret_cast<const bf16x8 *>(kbA + a_row + mt * 2048 + c1);
            }
            __builtin_amdgcn_sched_barrier(0);
            G8_P(1);
            // the reads are retired BEFORE the barrier (their latency has passed under the DMA issue): the other group may
            // restage these slots right after it
            G8_P(2);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            G8_P(3);
            __builtin_amdgcn_s_barrier();
            G8_P(4);
            G8_T(3 + (kt < 3 ? kt : 3), seq == 3 && kt < 4);   // first barrier of k-tiles 0..3 of tile 3
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt) {
                        acc[0][0][mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf0[nt][ks], af0[mt][ks], acc[0][0][mt][nt], 0, 0, 0);
                        acc[0][1][mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf1[nt][ks], af0[mt][ks], acc[0][1][mt][nt], 0, 0, 0);
                    }
            __builtin_amdgcn_s_setprio(0);
            G8_P(5);
            __builtin_amdgcn_s_barrier();
            G8_P(6);
            // ---------------- phase 2: A_1 (into the registers A_0 was in) -> Q(1,0), Q(1,1)
            // Group 0: the other 8 - N1 pieces of activation k-tile T+2; then everything but those eight must have landed:
            // k-tile T+1, whose last piece went out four intervals ago.  Group 1: the first 8 - N1 pieces of weight k-tile T+2
            // (slots of T: both groups retired their reads of it before phase 1's barriers); then all but these must have
            // landed: k-tile T+1.  A tile's first k-tile waits for nothing: what it needs was drained before the previous
            // epilogue, and a counted wait would also wait for that epilogue's stores (one in-order queue per wave).
            const bool live2 = h_left > 0 && !lastk;
            if (live2) {
                h_left -= N2;
#pragma unroll
                for (int i = 0; i < N2; ++i) issue_piece();
            }
            if constexpr (RL) {
                if (lastk) {   // R2: the weight slot of THIS k-tile (both groups retired their reads of it before phase 1's barriers)
                    rl_issue_sb(0, 1, R2);
                    rl_issue_sb(0, 2, R2 + 2048);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            G8_P(13);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                af0[mt][0] = *reinterpret_cast<const bf16x8 *>(kbA + 16384 + a_row + mt * 2048 + c0);
                af0[mt][1] = *reinterpret_cast<const bf16x8 *>(kbA + 16384 + a_row + mt * 2048 + c1);
            }
            __builtin_amdgcn_sched_barrier(0);
            G8_P(7);
            if (lastk) {
                // (RL: nothing is waited for here -- k-tile T+1 is the NEXT tile's first, read behind the epilogue, whose first
                // counted wait covers everything older; a wait here would stall the k-loop on the residual's HBM latency)
            } else if (kt) {
                if (!live2) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                else if (wr == 0) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
                else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N2) : "memory");
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            G8_P(8);
            __builtin_amdgcn_s_barrier();
            G8_P(9);
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt) {
                        acc[1][0][mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf0[nt][ks], af0[mt][ks], acc[1][0][mt][nt], 0, 0, 0);
                        acc[1][1][mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf1[nt][ks], af0[mt][ks], acc[1][1][mt][nt], 0, 0, 0);
                    }
            __builtin_amdgcn_s_setprio(0);
            G8_P(10);
            __builtin_amdgcn_s_barrier();
            G8_P(11);
            a_cur = a_cur == 2 ? 0 : a_cur + 1;
            w_cur ^= 1;
        }
        G8_T(8, seq == 2 && true);                   // end of the k-loop of tile 2 (before align)
        if (wr == 0) __builtin_amdgcn_s_barrier();   // group 0 meets group 1's last barrier of the tile
        G8_T(0, seq == 2);
        // Every read of the tile has been retired: complete the next tile's k-tile 1 (its W halves) now and drain the DMA
        // queue BEFORE the epilogue's stores go out.  Loads, stores and DMA share one in-order counter: a counted wait
        // behind the stores would hold the next tile's k-loop until they have all been acknowledged; this way the first
        // wait behind them comes a whole k-tile later.
        // (RL: nothing -- the next tile's k-tile 1 is staged from inside the epilogue, whose first counted wait covers k-tile 0)
        if constexpr (!RL) {
            if (wr == 0) issue_pieces(n8ktag);   // the next tile's weight k-tile 1 (slots of this tile's last k-tile)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        G8_T(1, seq == 2);

        // ---------------- epilogue, straight from the accumulators (the next tile's first k-tiles are already in LDS or in flight)
#ifdef G8_NO_EPI
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt) asm volatile("" ::"v"(acc[i][j][mt][nt]));
        continue;
#endif
        {
            const int colg = 8 * ((kg & 1) * 2 + (kg >> 1));   // after swap16: this lane's eight consecutive features inside a 32-column band
            // Loads first, stores last: a load issued behind a store waits for that store to retire (loads and stores share
            // vmcnt, in order), which serialises the epilogue on HBM write latency.
            if constexpr (RL) {
                // ---- RESID epilogue, residual through LDS (round 5).
                // Round 4's form loads a 128-row band of the residual into registers, computes it in place, loads the next band,
                // computes, stores: two HBM latencies in front of ~10 k cycles of arithmetic, and 24 stores issued in a row behind
                // it (~4 k cycles: 128 KiB through the CU's 64-B/clk memory pipe) -- 30-35 k cycles per tile, a whole K = 768
                // k-loop; every re-ordering of the loads died on VGPR spills (LABNOTES, round 4).  Here nothing the epilogue reads
                // passes through registers on its way in: each wave fetches ITS OWN 64 x 64 patch of the residual, its rows'
                // (mean, rstd) and its columns' (bias, gamma, beta) by LDS-DMA into a private region and reads them back with
                // ds_reads, and each sub-band's stores go out as soon as it is computed.  The LDS comes from the rings: the last
                // k-tile of a tile no longer stages the next tile's k-tile 1 (lastk in the k-loop), which leaves
                //   R1 = activation slot of the next tile's k-tile 1   (free during the whole last k-tile)
                //   R2 = weight slot of the same                        (free from phase 2 of the last k-tile)
                //   R3 = activation slot of the k-tile just read        (free from here)
                // i.e. 4 KiB of each per wave.  A sub-band s = (i, mt) is the wave's 16 rows x 64 columns (2 KiB = two DMA
                // instructions, one per 32-column band j).  Issue order of a wave (S = a sub-band's three stores; group 0 carries the
                // 8 activation pieces A, group 1 the 8 weight pieces W of the next tile's k-tile 1, staged behind a barrier as soon
                // as every wave is done with R1 / R2):
                //   last k-tile, phase 1:  stats cols sb0 -> R1        phase 2:  sb1 sb2 -> R2
                //   epilogue:  sb3 sb4 -> R3 | wait, registers <- stats, cols | sb0, S0 | barrier, A | sb1, sb5 -> R2, S1 |
                //              sb2, sb6 -> R2, S2 | sb3, sb7 -> R3, S3 | sb4, S4 | sb5, S5 | sb6, S6 | registers <- sb7 | barrier, W | sb7, S7 | wait(A / W)
                // Positions in a wave's in-order queue, from which every counted wait below is derived:
                //   group 1:  st 1, cols 2, sb0 3-4, sb1 5-6, sb2 7-8, sb3 9-10, sb4 11-12, S0 13-15, sb5 16-17, S1 18-20, sb6 21-22,
                //             S2 23-25, sb7 26-27, S3 28-30, S4 31-33, S5 34-36, S6 37-39, W 40-47, S7 48-50
                //   group 0:  ... S0 13-15, A 16-23, sb5 24-25, S1 26-28, sb6 29-30, S2 31-33, sb7 34-35, S3 36-38, ... S7 48-50
                // e.g. sb3 (10) is waited for behind S2 with vmcnt(25 - 10) = 15, or vmcnt(33 - 10) = 23 on a wave that has staged
                // A.  Only the last wait of group 1 (W sits behind S0..S6) covers stores younger than a few thousand cycles.
                // LDS layout of a sub-band instruction (band j): consumer lane (m16, kg) reads the 16-byte piece at
                // j*1024 + nt*512 + ((kg >> 1)*16 + m16)*16 and keeps the half kg & 1 -- its four features of tile nt: no lane
                // exchange on the way in.  (8-byte reads would do, but two of them get merged into a ds_read2 form, and hipcc puts
                // a vmcnt(0) in front of THAT -- it cannot tell which LDS-DMA it may alias -- which would serialize the pipeline.)
                const bool lo8 = m16 < 8;
                const unsigned lane_b = (unsigned)((wr * 64 + (m16 & 7)) * H + wc * 64 + (m16 >> 3) * 32 + colg);
                const unsigned rd_off = (unsigned)(((kg >> 1) * 16 + m16) * 16);
                const bool rd_hi = kg & 1;
#define G8_VM(n) asm volatile("s_waitcnt vmcnt(" #n ")" ::: "memory")
#define G8_VMC(c, a, b) do { if (c) G8_VM(a); else G8_VM(b); } while (0)
#define G8_LDS_DONE() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
                constexpr std::integral_constant<int, -1> cnone{};
                constexpr std::integral_constant<int, 0> c0t{};
                constexpr std::integral_constant<int, 1> c1t{};
                constexpr std::integral_constant<int, 2> c2t{};
                constexpr std::integral_constant<int, 3> c3t{};
                constexpr std::integral_constant<int, 8> n8tag{};
                rl_issue_sb(0, 3, R3);
                rl_issue_sb(1, 0, R3 + 2048);
                G8_E(0);
                G8_VM(8);                                     // stats, cols, sb0 -- and everything older: the next tile's k-tile 0
                G8_E(1);
                float mean_[2][4], rstd_[2][4];
                f4v rg[2][2], rb[2][2];                       // [j][nt]
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int mt = 0; mt < 4; ++mt) {
                        // the 16 bytes that hold the statistics of rows m16 & ~1 and m16 | 1 (8-byte reads would be merged, see above)
                        g8_u4 c = *reinterpret_cast<const g8_u4 *>(R1 + i * 512 + (mt * 16 + (m16 & 14)) * 8);
                        asm volatile("" : "+v"(c));
                        // (each its own register: a broadcast of a pair's high word into packed fp32 arithmetic would be the
                        // `op_sel` form of tools/probes/pk_after_load_probe.hip)
                        asm volatile("v_mov_b32 %0, %1" : "=v"(mean_[i][mt]) : "v"((m16 & 1) ? c.z : c.x));
                        asm volatile("v_mov_b32 %0, %1" : "=v"(rstd_[i][mt]) : "v"((m16 & 1) ? c.w : c.y));
                    }
#pragma unroll
                for (int jj = 0; jj < 2; ++jj)
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt) {
                        const int co = (jj * 32 + nt * 16 + 4 * kg) * 4;
                        // the bias goes into the accumulators here (acc + bias + (...) is evaluated in this order anyway): sixteen
                        // registers fewer to hold through the epilogue -- with them it spilled
                        const f4v cvv = *reinterpret_cast<const f4v *>(R1 + 1024 + co);
#pragma unroll
                        for (int i = 0; i < 2; ++i)
#pragma unroll
                            for (int mt = 0; mt < 4; ++mt) acc[i][jj][mt][nt] += cvv;
                        rg[jj][nt] = *reinterpret_cast<const f4v *>(R1 + 1024 + 256 + co);
                        rb[jj][nt] = *reinterpret_cast<const f4v *>(R1 + 1024 + 512 + co);
                    }
                // one sub-band: read, compute, (refill its region with sub-band (1, refill)), its three stores
                auto sb_read = [&](const unsigned char *sb, g8_u4 (&c)[2][2]) __attribute__((always_inline)) {
#pragma unroll
                    for (int jj = 0; jj < 2; ++jj) {
                        c[jj][0] = *reinterpret_cast<const g8_u4 *>(sb + jj * 1024 + rd_off);
                        c[jj][1] = *reinterpret_cast<const g8_u4 *>(sb + jj * 1024 + 512 + rd_off);
                        // (the whole vector is "used": otherwise the load is narrowed to two 8-byte halves and re-merged by the backend)
                        asm volatile("" : "+v"(c[jj][0]), "+v"(c[jj][1]));
                    }
                };
                auto sb_do = [&](auto itag, auto mttag, unsigned char *sb, auto refilltag, const g8_u4 (*pre)[2]) __attribute__((always_inline)) {
                    constexpr int i = decltype(itag)::value, mt = decltype(mttag)::value, refill = decltype(refilltag)::value;
                    const float mean = mean_[i][mt], rstd = rstd_[i][mt];
                    uint4 ro[2];
                    float s1 = 0.f, s2 = 0.f;
                    g8_u4 cc[2][2];
                    if (pre) {
#pragma unroll
                        for (int jj = 0; jj < 2; ++jj) cc[jj][0] = pre[jj][0], cc[jj][1] = pre[jj][1];
                    } else {
                        sb_read(sb, cc);
                    }
#pragma unroll
                    for (int jj = 0; jj < 2; ++jj) {
                        const g8_u4 c0 = cc[jj][0], c1 = cc[jj][1];
                        const uint2 w0 = {rd_hi ? c0.z : c0.x, rd_hi ? c0.w : c0.y}, w1 = {rd_hi ? c1.z : c1.x, rd_hi ? c1.w : c1.y};
                        const f4v ra = {__uint_as_float(w0.x << 16), __uint_as_float(w0.x & 0xffff0000u), __uint_as_float(w0.y << 16), __uint_as_float(w0.y & 0xffff0000u)};
                        const f4v rb_ = {__uint_as_float(w1.x << 16), __uint_as_float(w1.x & 0xffff0000u), __uint_as_float(w1.y << 16), __uint_as_float(w1.y & 0xffff0000u)};
                        const f4v o0 = acc[i][jj][mt][0] + ((ra - mean) * rstd * rg[jj][0] + rb[jj][0]);
                        const f4v o1 = acc[i][jj][mt][1] + ((rb_ - mean) * rstd * rg[jj][1] + rb[jj][1]);
                        unsigned p0 = pack_bf16(o0.x, o0.y), p1 = pack_bf16(o0.z, o0.w);
                        unsigned p2 = pack_bf16(o1.x, o1.y), p3 = pack_bf16(o1.z, o1.w);
                        swap16(p0, p2);
                        swap16(p1, p3);
                        ro[jj] = make_uint4(p0, p1, p2, p3);
                        const f4v sm = o0 + o1, sq = o0 * o0 + o1 * o1;
                        const float t1 = (sm.x + sm.y) + (sm.z + sm.w), t2 = (sq.x + sq.y) + (sq.z + sq.w);
                        s1 = jj ? s1 + t1 : t1;
                        s2 = jj ? s2 + t2 : t2;
                    }
                    // the four lane groups of a row hold different features: add them (they are 16 lanes apart: ds_bpermute)
                    s1 += __shfl_xor(s1, 16);
                    s2 += __shfl_xor(s2, 16);
                    s1 += __shfl_xor(s1, 32);
                    s2 += __shfl_xor(s2, 32);
                    xchg8(ro[0], ro[1], lo8);   // (band 0, band 1) -> the two line-shaped stores
                    G8_LDS_DONE();              // every read of this sub-band's region has returned: it may be refilled
                    if constexpr (refill >= 0) rl_issue_sb(1, refill, sb);
                    __builtin_amdgcn_sched_barrier(0);
                    // the sub-band's THREE stores (the counted waits count them)
                    const size_t row = (size_t)m0 + i * 128 + wr * 64 + mt * 16 + m16;
#if defined(G8_RL_ABL) && (G8_RL_ABL & 1)   // timing only: the three stores with one lane each (same queue entries, no data)
                    if (lane == 0) g.part[row * (g.N >> 6) + (n0 >> 6) + wc] = make_float2(s1, s2);
#pragma unroll
                    for (int jj = 0; jj < 2; ++jj)
                        if (lane == 0) g8_store16<NT>(g.yb + rl_tb + (size_t)((i * 128 + mt * 16 + jj * 8) * H) + lane_b, ro[jj]);
#else
                    if (kg == 0) g.part[row * (g.N >> 6) + (n0 >> 6) + wc] = make_float2(s1, s2);   // one partial per (row, wave)
#pragma unroll
                    for (int jj = 0; jj < 2; ++jj)
                        g8_store16<NT>(g.yb + rl_tb + (size_t)((i * 128 + mt * 16 + jj * 8) * H) + lane_b, ro[jj]);
#endif
                    __builtin_amdgcn_sched_barrier(0);
                };
                __builtin_amdgcn_sched_barrier(0);
                bool gA = false, gW = false;                  // this wave has staged pieces of the next tile's k-tile 1 (no next tile: no)
                sb_do(c0t, c0t, R1 + 2048, cnone, nullptr);            // sb0 (the statistics and column vectors are in registers by now)
                G8_E(2);
                __builtin_amdgcn_s_barrier();                 // every wave is done with R1: the next tile's activation k-tile 1 may land there
                if (wr == 0) gA = issue_pieces(n8tag);
                __builtin_amdgcn_sched_barrier(0);
                G8_E(3);
                G8_VMC(gA, 17, 9);
                G8_E(4);
                sb_do(c0t, c1t, R2, c1t, nullptr);                     // sb1, then sb5 = (1, 1) into its region
                G8_VMC(gA, 20, 12);
                G8_E(5);
                sb_do(c0t, c2t, R2 + 2048, c2t, nullptr);              // sb2, sb6 = (1, 2)
                G8_VMC(gA, 23, 15);
                G8_E(6);
                sb_do(c0t, c3t, R3, c3t, nullptr);                     // sb3, sb7 = (1, 3)
                G8_VMC(gA, 26, 18);
                G8_E(7);
                sb_do(c1t, c0t, R3 + 2048, cnone, nullptr);            // sb4
                G8_VM(16);
                G8_E(8);
                sb_do(c1t, c1t, R2, cnone, nullptr);                   // sb5
                G8_VM(14);
                G8_E(9);
                sb_do(c1t, c2t, R2 + 2048, cnone, nullptr);            // sb6
                G8_E(10);
                // sb7 is taken out of R3 BEFORE the barrier: once past it a wave of group 0 may run into the next tile's first
                // phase, which stages that tile's k-tile 2 into R3's slot -- no barrier of the k-loop stands in between
                G8_VM(12);
                G8_E(11);
                g8_u4 c7[2][2];
                sb_read(R3, c7);
                G8_LDS_DONE();
                __builtin_amdgcn_s_barrier();                 // every wave is done with R2 and R3: the next tile's weight k-tile 1 may land
                if (wr == 1) gW = issue_pieces(n8tag);
                __builtin_amdgcn_sched_barrier(0);
                G8_E(12);
                sb_do(c1t, c3t, R3, cnone, c7);               // sb7 (from registers)
                G8_E(13);
                // the next tile's k-tile 1 has landed when its k-loop starts (its first k-tile waits for nothing): A is 27 entries
                // back in group 0's queue (every store behind it stays in flight), W three in group 1's
                G8_VMC(gW, 3, 27);
                G8_E(14);
                G8_E(15);
#undef G8_VM
#undef G8_VMC
#undef G8_LDS_DONE
            } else {
                float2 st[2][4];   // (mean, rstd) of the A rows
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int mt = 0; mt < 4; ++mt) st[i][mt] = g.astats[(size_t)m0 + i * 128 + wr * 64 + mt * 16 + m16];
                const int ldo = EPI == EPI8_GELU ? g.N : H;          // row pitch of the output
                const bool lo8 = m16 < 8;
                // memory side (q | k | h): lane (m16, kg) addresses row (m16 & 7) [+ 8] of a 16-row block, band m16 >> 3
                const unsigned lane_b = (unsigned)((wr * 64 + (m16 & 7)) * ldo + wc * 64 + (m16 >> 3) * 32 + colg);
                f4v ws[2][2], cv[2][2];   // [j][nt]
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt) {
                        const int nb = n0 + wc * 64 + j * 32;           // first column of the band
                        cv[j][nt] = *reinterpret_cast<const f4v *>(g.cvec + nb + nt * 16 + 4 * kg);
                        ws[j][nt] = *reinterpret_cast<const f4v *>(g.wsum + nb + nt * 16 + 4 * kg);
                    }
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int mt = 0; mt < 4; ++mt) {
                        const float nm = -st[i][mt].x * st[i][mt].y;   // rstd * (acc - mean * wsum) + c = rstd * acc + (c - mean * rstd * wsum)
                        // rstd is the HIGH word of the loaded (mean, rstd) pair: broadcast into packed fp32 arithmetic straight from there
                        // it becomes `v_pk_fma_f32 ... op_sel:[1,0,0]`, the form that gave a wrong low half beside other waves' MFMAs
                        // (tools/probes/pk_after_load_probe.hip).  Passed through an opaque copy it is a value of its own: the compiler
                        // broadcasts the LOW word of a fresh register (op_sel_hi), the form the probe never saw fail.
                        float rs = st[i][mt].y;
                        asm volatile("v_mov_b32 %0, %1" : "=v"(rs) : "v"(st[i][mt].y));
                        uint4 o[2];
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            const int nb = n0 + wc * 64 + j * 32;
                            unsigned p[4];
#pragma unroll
                            for (int nt = 0; nt < 2; ++nt) {
                                f4v v = acc[i][j][mt][nt] * rs + (ws[j][nt] * nm + cv[j][nt]);
                                if (EPI == EPI8_QKV && n0 >= 2 * H) {   // tile-uniform: the V projection
                                    // The attention kernel wants V token-contiguous: v16[token group of 16][feature][16 tokens].  The lane
                                    // holds four features of ONE token; a 4x4 transpose inside each quad of lanes (tokens 4a .. 4a+3) gives
                                    // it four tokens of ONE feature = 8 contiguous bytes of v16 (16 DPP / select ops per four values).
                                    quad_transpose4(v, lane & 3);
                                    const int n = nb + nt * 16 + 4 * kg + (lane & 3) - 2 * H;
                                    const size_t mg = (size_t)(m0 + i * 128 + wr * 64 + mt * 16) >> 4;
                                    uint2 o2;
                                    o2.x = pack_bf16(v.x, v.y);
                                    o2.y = pack_bf16(v.z, v.w);
                                    g8_store8<NT>(g.v16 + (mg * H + n) * 16 + (m16 & 12), o2);
                                    continue;
                                }
                                if constexpr (EPI == EPI8_GELU) {
                                    const f2v g0 = gelu8_2((f2v){v.x, v.y}), g1 = gelu8_2((f2v){v.z, v.w});
                                    p[2 * nt] = pack_bf16(g0.x, g0.y);
                                    p[2 * nt + 1] = pack_bf16(g1.x, g1.y);
                                } else {
                                    p[2 * nt] = pack_bf16(v.x, v.y);
                                    p[2 * nt + 1] = pack_bf16(v.z, v.w);
                                }
                            }
                            if (EPI == EPI8_QKV && n0 >= 2 * H) continue;   // V tile: already stored, token-contiguous
                            swap16(p[0], p[2]);
                            swap16(p[1], p[3]);
                            o[j] = make_uint4(p[0], p[1], p[2], p[3]);
                        }
                        if (EPI == EPI8_QKV && n0 >= 2 * H) continue;
                        xchg8(o[0], o[1], lo8);   // two line-shaped stores: rows 0..7 and 8..15 of the block, 128 bytes each
                        const size_t ur = (size_t)(m0 + i * 128 + mt * 16) * ldo;
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            if constexpr (EPI == EPI8_GELU) {
                                g8_store16<NT>(g.h + ur + (size_t)(j * 8) * ldo + n0 + lane_b, o[j]);
                            } else {   // q | k: columns [0, 768) are Q (the softmax scale log2(e)/8 is folded into its weights), [768, 1536) K
                                bf16 *dst = n0 < H ? g.q + ur + n0 : g.k + ur + (n0 - H);
                                g8_store16<NT>(dst + (size_t)(j * 8) * ldo + lane_b, o[j]);
                            }
                        }
                    }
            }
        }
    }
    if constexpr (EPI == EPI8_GELU) {
        if (g.clk && blockIdx.x == 0 && tid == 0) {
            g.clk[2] = __builtin_amdgcn_s_memtime();
            g.clk[3] = __builtin_amdgcn_s_memrealtime();
        }
    }
#ifdef G8_STAMP2
    if (blockIdx.x == 8 && lane == 0 && (w == 0 || w == 4)) {
        unsigned long long *o = reinterpret_cast<unsigned long long *>(g.part) + 64 + (w ? 16 : 0);
        for (int i = 0; i < 16; ++i) o[i] = ph[i];
    }
#endif
#ifdef G8_STAMP
    if (blockIdx.x == 8 && lane == 0 && (w == 0 || w == 4)) {
        unsigned long long *o = reinterpret_cast<unsigned long long *>(g.part) + (w ? 16 : 0);
        for (int i = 0; i < 16; ++i) o[i] = stamps[i];
        for (int i = 0; i < 16; ++i) o[32 + i] = est[i];
    }
#endif
}

// (sum, sum of squares) partials of a row (one per 64 columns) -> (mean, rstd)
__global__ __launch_bounds__(256) void ln_combine_kernel(const float2 *__restrict__ part, int n_part, int n_cols, const int *__restrict__ total_rows,
                                                         float eps, float2 *__restrict__ stats) {
    const size_t row = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= (size_t)((*total_rows + 255) & ~255)) return;
    float s1 = 0.f, s2 = 0.f;
    if ((n_part & 1) == 0) {   // 16-byte loads, all issued before the first add (a row's partials are 96 contiguous bytes at N = 768)
        const float4 *p4 = reinterpret_cast<const float4 *>(part + row * n_part);
        float4 v[8];
        const int n4 = n_part >> 1;
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = i < n4 ? p4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            s1 += v[i].x + v[i].z;
            s2 += v[i].y + v[i].w;
        }
        for (int i = 16; i < n_part; ++i) {
            const float2 p = part[row * n_part + i];
            s1 += p.x;
            s2 += p.y;
        }
    } else {
        for (int i = 0; i < n_part; ++i) {
            const float2 p = part[row * n_part + i];
            s1 += p.x;
            s2 += p.y;
        }
    }
    const float mean = s1 / n_cols;
    const float var = fmaxf(s2 / n_cols - mean * mean, 0.f);
    stats[row] = make_float2(mean, rsqrtf(var + eps));
}

// W' = W . diag(gamma) * scale (bf16), wsum[n] = sum_k W'[n,k] (of the rounded values: what the MFMA multiplies by),
// cvec[n] = (bias[n] + sum_k beta[k] W[n,k]) * scale.  gamma / beta null: plain conversion, wsum = 0, cvec = bias * scale.
__global__ __launch_bounds__(256) void fold_ln_kernel(const float *__restrict__ Wf, const float *__restrict__ bias, const float *__restrict__ gamma,
                                                      const float *__restrict__ beta, int K, float scale, bf16 *__restrict__ Wb,
                                                      float *__restrict__ wsum, float *__restrict__ cvec) {
    __shared__ float red[2][4];
    const int n = blockIdx.x, tid = threadIdx.x;
    float s = 0.f, c = 0.f;
    for (int k = tid; k < K; k += 256) {
        const float wv = Wf[(size_t)n * K + k];
        const bf16 wb = (bf16)(wv * (gamma ? gamma[k] : 1.f) * scale);
        Wb[(size_t)n * K + k] = wb;
        s += (float)wb;
        if (beta) c += beta[k] * wv;
    }
    s = wave_sum(s);
    c = wave_sum(c);
    if ((tid & 63) == 0) {
        red[0][tid >> 6] = s;
        red[1][tid >> 6] = c;
    }
    __syncthreads();
    if (tid == 0) {
        wsum[n] = gamma ? (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]) : 0.f;
        cvec[n] = (bias[n] + (red[1][0] + red[1][1]) + (red[1][2] + red[1][3])) * scale;
    }
}

__global__ void fill_identity_stats_kernel(float2 *__restrict__ stats, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) stats[i] = make_float2(0.f, 1.f);
}
