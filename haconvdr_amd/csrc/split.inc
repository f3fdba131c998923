// Split-bf16 precision mode (hac_encoder_set_option "precision" = "split"), included by encoder.hip.
//
// Every operand of every matrix product is a PAIR of bf16 values, hi = bf16(v) and lo = bf16(v - float(hi)), and a product
// a.b is accumulated as a_lo.b_hi + a_hi.b_lo + a_hi.b_hi, in that order, into the fp32 accumulator (the lo.lo term, 2^-18
// relative, is dropped): the operand error goes from 2^-9 to 2^-17 relative at three bf16 MFMAs per product.  A twin tensor
// has the layout of its hi tensor, so every address formula, swizzle and LDS-DMA piece of the bf16 kernels is reused with a
// second base pointer.  Residual stream, LayerNorm, softmax and head are fp32, as in the classic family.

// the pair's defining helper (host twin: haconvdr_amd.encoder.split_bf16)
__device__ __forceinline__ void split_bf16(float v, bf16 &hi, bf16 &lo) {
    hi = (bf16)v;
    lo = (bf16)(v - (float)hi);
}

// lo twin of a tensor whose fp32 values are at hand: packed weights (from the checkpoint's fp32 copy) and the embedding rows
__global__ void f32_to_bf16_lo_kernel(const float *__restrict__ src, bf16 *__restrict__ dst, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        bf16 hi, lo;
        split_bf16(src[i], hi, lo);
        dst[i] = lo;
    }
}

// LayerNorm of the packed rows behind a RESID GEMM, both forms of the classic family in one kernel: the deferred form
// (ln_stats_rows_kernel: statistics + the next GEMM's A operand, here as a pair; split-K slices added up in slice order) when
// stats is given, the plain form of the compact tail (ln_rows_kernel: the fp32 rows too) when x_f32 is.
__global__ __launch_bounds__(256) void ln_split_rows_kernel(float *__restrict__ y, const int *__restrict__ total_rows,
                                                            const float *__restrict__ gamma, const float *__restrict__ beta, float eps,
                                                            float2 *__restrict__ stats, float *__restrict__ x_f32, bf16 *__restrict__ x_hi,
                                                            bf16 *__restrict__ x_lo, const float *__restrict__ part, int n_part, size_t part_stride) {
    const int lane = threadIdx.x & 63;
    const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (size_t)*total_rows) return;
    float v[12];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        f4v a = *reinterpret_cast<const f4v *>(y + row * H + i * 256 + lane * 4);
        for (int sp = 0; sp < n_part; ++sp) a += *reinterpret_cast<const f4v *>(part + sp * part_stride + row * H + i * 256 + lane * 4);
        if (n_part) *reinterpret_cast<f4v *>(y + row * H + i * 256 + lane * 4) = a;
        v[i * 4 + 0] = a.x;
        v[i * 4 + 1] = a.y;
        v[i * 4 + 2] = a.z;
        v[i * 4 + 3] = a.w;
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 12; ++i) s += v[i];
    const float mean = wave_sum(s) * (1.0f / H);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        const float d = v[i] - mean;
        q += d * d;
    }
    const float rstd = rsqrtf(wave_sum(q) * (1.0f / H) + eps);
    if (stats && lane == 0) stats[row] = make_float2(mean, rstd);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int c = i * 256 + lane * 4;
        const f4v g = *reinterpret_cast<const f4v *>(gamma + c);
        const f4v bb = *reinterpret_cast<const f4v *>(beta + c);
        float o[4];
        o[0] = (v[i * 4 + 0] - mean) * rstd * g.x + bb.x;
        o[1] = (v[i * 4 + 1] - mean) * rstd * g.y + bb.y;
        o[2] = (v[i * 4 + 2] - mean) * rstd * g.z + bb.z;
        o[3] = (v[i * 4 + 3] - mean) * rstd * g.w + bb.w;
        if (x_f32) *reinterpret_cast<f4v *>(x_f32 + row * H + c) = (f4v){o[0], o[1], o[2], o[3]};
        bf16x4 oh, ol;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            bf16 hi, lo;
            split_bf16(o[j], hi, lo);
            oh[j] = hi;
            ol[j] = lo;
        }
        *reinterpret_cast<bf16x4 *>(x_hi + row * H + c) = oh;
        *reinterpret_cast<bf16x4 *>(x_lo + row * H + c) = ol;
    }
}

// ------------------------------------------------------------------ split GEMM  C = A[M,K] . W[N,K]^T  (+ fused epilogue)
struct GemmSplitArgs {
    GemmArgs g;                   // the hi tensors and everything fp32, as the classic kernel takes them
    const bf16 *A_lo, *W_lo;
    bf16 *q_lo, *k_lo, *v16_lo;   // EPI_QKV
    bf16 *h_lo;                   // EPI_GELU
};

// erf GELU good to fp32: the classic epilogue's degree-8 polynomial (7.4e-5 absolute, 2^-13 relative) would be sixteen times
// the error of the operands this mode feeds the next GEMM
__device__ __forceinline__ float gelu_erf_f32(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752f)); }

// Modelled on gemm_bf16_nt_kernel<EPI, 2>: 128 x 128 x 64 tiles, 4 waves (2 x 2), persistent over XCD-aware tile runs, LDS-DMA
// staging into the same XOR-swizzled image, split-K for the RESID class, the same transposing epilogues.  A stage holds four
// operand tiles (A_hi, A_lo, W_hi, W_lo: 64 KiB); two stages and the four transpose patches are 144 KiB of the CU's 160 KiB:
// one workgroup per CU.  The 256 x 256 form would need two stages of 128 KiB and was not built: this kernel is bound by
// L2 -> LDS traffic at twice the classic kernel's staged bytes per flop-triple, which is what the mode's cost above 3 x is.
constexpr int SPLIT_GEMM_LDS = 2 * 4 * 128 * 128 + 4 * 4096;   // two stages of four operand tiles + the per-wave patches
template <int EPI>
__global__ __launch_bounds__(256, 1) void gemm_split_nt_kernel(GemmSplitArgs ga) {
    constexpr int BM = 128, BN = 128;
    constexpr int TILE = BM * 128;         // bytes of one operand tile (128 rows x 64 bf16)
    constexpr int STAGE = 4 * TILE;        // A_hi | A_lo | W_hi | W_lo
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const GemmArgs &g = ga.g;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int K = g.K, KT = K / BK;
    const int nx = g.N / BN;
    const int S = (EPI == EPI_RESID && g.ksplit > 1) ? g.ksplit : 1, KTs = KT / S;
    const int n_tiles = ((*g.total_rows + BM - 1) / BM) * nx * S;
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, per_xcd = (gridDim.x + 7 - xcd) >> 3;
    const int run_lo = (int)((long)n_tiles * xcd / 8), run_hi = (int)((long)n_tiles * (xcd + 1) / 8);
    int tile = run_lo + slot;
    if (tile >= run_hi) return;
    const int wm = w >> 1, wn = w & 1;
    const int r = lane & 31, hh = lane >> 5;

    typedef const __attribute__((address_space(1))) void *gvp;
    typedef __attribute__((address_space(3))) void *lvp;
    const int srow = lane >> 3;
    const int sch_even = (lane & 7) ^ (srow >> 1), sch_odd = sch_even ^ 4;
    const size_t lane_src_e = (size_t)(w * 32 + srow) * K + sch_even * 8;
    const size_t lane_src_o = (size_t)(w * 32 + srow) * K + sch_odd * 8;
    auto stage = [&](int buf, int t, int kt) {   // kt: absolute k-tile
        const int tt = EPI == EPI_RESID ? t / S : t;
        const size_t ao = (size_t)((tt / nx) * BM) * K + kt * BK, wo = (size_t)((tt % nx) * BN) * K + kt * BK;
        unsigned char *sb = smem + buf * STAGE + w * 4096;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const size_t ls = ((i & 1) ? lane_src_o : lane_src_e) + (size_t)i * 8 * K;
            __builtin_amdgcn_global_load_lds((gvp)(g.A + ao + ls), (lvp)(sb + i * 1024), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((gvp)(ga.A_lo + ao + ls), (lvp)(sb + TILE + i * 1024), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((gvp)(g.W + wo + ls), (lvp)(sb + 2 * TILE + i * 1024), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((gvp)(ga.W_lo + wo + ls), (lvp)(sb + 3 * TILE + i * 1024), 16, 0, 0);
        }
    };
    int aoff[2], woff[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) aoff[t] = (wm * 64 + t * 32 + r) * 128;
#pragma unroll
    for (int t = 0; t < 2; ++t) woff[t] = 2 * TILE + (wn * 64 + t * 32 + r) * 128;
    const int sw = (r >> 1) & 7;
    float *patch = reinterpret_cast<float *>(smem + 2 * STAGE) + w * 1024;  // [16 rows][64 cols] fp32, wave-private

    int cur = 0;
    stage(0, tile, EPI == EPI_RESID ? (tile % S) * KTs : 0);
    __syncthreads();
    for (; tile < run_hi; tile += per_xcd) {
        const int otile = EPI == EPI_RESID ? tile / S : tile, slice = EPI == EPI_RESID ? tile - otile * S : 0, kb = slice * KTs;
        const int m0 = (otile / nx) * BM, n0 = (otile % nx) * BN;
        const int next_tile = tile + per_xcd;
        f32x16 acc[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;

        for (int kt = 0; kt < KTs; ++kt) {
            if (kt + 1 < KTs) stage(cur ^ 1, tile, kb + kt + 1);
            else if (next_tile < run_hi) stage(cur ^ 1, next_tile, EPI == EPI_RESID ? (next_tile % S) * KTs : 0);
            const unsigned char *sc = smem + cur * STAGE;
            bf16x8 ah[2][2], al[2][2], wh[2][2], wl[2][2];   // [fragment buffer][32-row tile]
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                ah[0][t] = *reinterpret_cast<const bf16x8 *>(sc + aoff[t] + ((hh ^ sw) << 4));
                al[0][t] = *reinterpret_cast<const bf16x8 *>(sc + TILE + aoff[t] + ((hh ^ sw) << 4));
                wh[0][t] = *reinterpret_cast<const bf16x8 *>(sc + woff[t] + ((hh ^ sw) << 4));
                wl[0][t] = *reinterpret_cast<const bf16x8 *>(sc + TILE + woff[t] + ((hh ^ sw) << 4));
            }
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                if (ks < 3) {
                    const int c = (((ks + 1) * 2 + hh) ^ sw) << 4;
#pragma unroll
                    for (int t = 0; t < 2; ++t) {
                        ah[(ks + 1) & 1][t] = *reinterpret_cast<const bf16x8 *>(sc + aoff[t] + c);
                        al[(ks + 1) & 1][t] = *reinterpret_cast<const bf16x8 *>(sc + TILE + aoff[t] + c);
                        wh[(ks + 1) & 1][t] = *reinterpret_cast<const bf16x8 *>(sc + woff[t] + c);
                        wl[(ks + 1) & 1][t] = *reinterpret_cast<const bf16x8 *>(sc + TILE + woff[t] + c);
                    }
                }
                // one fixed order per fragment pair and k-step: lo.hi, hi.lo, hi.hi
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int b = 0; b < 2; ++b) {
                        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[ks & 1][a], wh[ks & 1][b], acc[a][b], 0, 0, 0);
                        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[ks & 1][a], wl[ks & 1][b], acc[a][b], 0, 0, 0);
                        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[ks & 1][a], wh[ks & 1][b], acc[a][b], 0, 0, 0);
                    }
            }
            __syncthreads();  // hipcc drains the LDS-DMA (vmcnt(0)) here: next stage landed, this one is free
            cur ^= 1;
        }

        // ---- epilogue: the classic kernel's (acc[a][b][e] is element m = m0 + wm*64 + a*32 + (e&3) + 8*(e>>2) + 4*hh,
        // n = n0 + wn*64 + b*32 + r), writing pairs where that one writes bf16
        const int ncol0 = n0 + wn * 64;
        const bool partial = EPI == EPI_RESID && slice > 0;
        const float bias0 = partial ? 0.f : g.bias[ncol0 + r], bias1 = partial ? 0.f : g.bias[ncol0 + 32 + r];
        [[maybe_unused]] float *const y_out = partial ? g.part + (size_t)(slice - 1) * g.part_stride : g.y;
        if (EPI == EPI_QKV && n0 >= 2 * H) {   // V in 16-key groups: a lane holds 4 consecutive tokens of one feature
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const int n = ncol0 + b * 32 + r - 2 * H;
                const float bias = b ? bias1 : bias0;
#pragma unroll
                for (int a = 0; a < 2; ++a) {
                    const size_t mg = (size_t)(m0 + wm * 64 + a * 32) >> 4;
#pragma unroll
                    for (int e4 = 0; e4 < 4; ++e4) {
                        bf16x4 oh, ol;
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            float v = acc[a][b][e4 * 4 + j] + bias;
                            asm volatile("" : "+v"(v));   // (one value, one VGPR: no packed-fp32 forms, see the RESID epilogue of the classic kernel)
                            bf16 hi, lo;
                            split_bf16(v, hi, lo);
                            oh[j] = hi;
                            ol[j] = lo;
                        }
                        const size_t o = ((mg + (e4 >> 1)) * H + n) * 16 + 8 * (e4 & 1) + 4 * hh;
                        *reinterpret_cast<bf16x4 *>(g.v16 + o) = oh;
                        *reinterpret_cast<bf16x4 *>(ga.v16_lo + o) = ol;
                    }
                }
            }
            continue;
        }
#pragma unroll
        for (int a = 0; a < 2; ++a) {
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                f4v rs[4];
                if constexpr (EPI == EPI_RESID) {
                    const size_t mr = (size_t)m0 + wm * 64 + a * 32 + half * 16;
#pragma unroll
                    for (int it = 0; it < 4; ++it)
                        rs[it] = partial ? (f4v){0.f, 0.f, 0.f, 0.f} : *reinterpret_cast<const f4v *>(g.resid + (mr + it * 4 + (lane >> 4)) * H + ncol0 + (lane & 15) * 4);
                    if (g.rstats && !partial) {   // deferred LayerNorm of the residual rows
                        const f4v gam = *reinterpret_cast<const f4v *>(g.rgamma + ncol0 + (lane & 15) * 4);
                        const f4v bet = *reinterpret_cast<const f4v *>(g.rbeta + ncol0 + (lane & 15) * 4);
#pragma unroll
                        for (int it = 0; it < 4; ++it) {
                            const float2 st = g.rstats[mr + it * 4 + (lane >> 4)];
                            // (values pinned to VGPRs of their own: no packed-fp32 op_sel forms, as in the classic kernel)
                            float c0 = rs[it].x, c1 = rs[it].y, c2 = rs[it].z, c3 = rs[it].w, mean = st.x, rstd = st.y;
                            asm volatile("" : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3), "+v"(mean), "+v"(rstd));
                            c0 = fmaf((c0 - mean) * rstd, gam.x, bet.x);
                            c1 = fmaf((c1 - mean) * rstd, gam.y, bet.y);
                            c2 = fmaf((c2 - mean) * rstd, gam.z, bet.z);
                            c3 = fmaf((c3 - mean) * rstd, gam.w, bet.w);
                            asm volatile("" : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3));
                            rs[it] = (f4v){c0, c1, c2, c3};
                        }
                    }
                }
#pragma unroll
                for (int e8 = 0; e8 < 8; ++e8) {
                    const int e = half * 8 + e8;
                    const int row = (e8 & 3) + 8 * (e8 >> 2) + 4 * hh;   // 0..15
                    patch[row * 64 + r] = acc[a][0][e] + bias0;
                    patch[row * 64 + 32 + r] = acc[a][1][e] + bias1;
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): the wave's own LDS writes have landed
                __builtin_amdgcn_wave_barrier();
                const size_t mrow = (size_t)m0 + wm * 64 + a * 32 + half * 16;
                if constexpr (EPI == EPI_RESID) {
#pragma unroll
                    for (int it = 0; it < 4; ++it) {
                        const int row = it * 4 + (lane >> 4), c4 = (lane & 15) * 4;
                        const f4v v = *reinterpret_cast<const f4v *>(patch + row * 64 + c4);
                        const size_t off = (mrow + row) * H + ncol0 + c4;
                        *reinterpret_cast<f4v *>(y_out + off) = v + rs[it];
                    }
                } else {
                    // Q is scaled by log2(e)/sqrt(64) in fp32 before the pair is formed (the softmax runs in base 2)
                    const float sc = (EPI == EPI_QKV && n0 < H) ? 0.125f * 1.44269504088896341f : 1.0f;
#pragma unroll
                    for (int it = 0; it < 2; ++it) {
                        const int row = it * 8 + (lane >> 3), c8 = (lane & 7) * 8;
                        const f4v v0 = *reinterpret_cast<const f4v *>(patch + row * 64 + c8);
                        const f4v v1 = *reinterpret_cast<const f4v *>(patch + row * 64 + c8 + 4);
                        const float in[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
                        bf16x8 oh, ol;
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            float v = in[j];
                            asm volatile("" : "+v"(v));
                            if constexpr (EPI == EPI_GELU) v = gelu_erf_f32(v);
                            else v = v * sc;
                            asm volatile("" : "+v"(v));
                            bf16 hi, lo;
                            split_bf16(v, hi, lo);
                            oh[j] = hi;
                            ol[j] = lo;
                        }
                        if constexpr (EPI == EPI_GELU) {
                            const size_t o = (mrow + row) * (size_t)g.N + ncol0 + c8;
                            *reinterpret_cast<bf16x8 *>(g.h + o) = oh;
                            *reinterpret_cast<bf16x8 *>(ga.h_lo + o) = ol;
                        } else {
                            const size_t o = (mrow + row) * H + (n0 < H ? ncol0 : ncol0 - H) + c8;
                            *reinterpret_cast<bf16x8 *>((n0 < H ? g.q : g.k) + o) = oh;
                            *reinterpret_cast<bf16x8 *>((n0 < H ? ga.q_lo : ga.k_lo) + o) = ol;
                        }
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                __builtin_amdgcn_s_waitcnt(0xC07F);  // reads done before the next sub-tile overwrites the patch
                __builtin_amdgcn_wave_barrier();
            }
        }
    }
}

// ------------------------------------------------------------------ split attention
struct AttnSplitArgs {
    const bf16 *q, *q_lo, *k, *k_lo;   // q (pre-scaled by log2(e)/8), k: [Mp][768]
    const bf16 *v16, *v16_lo;          // V in 16-key groups: [Mp/16][768][16]
    bf16 *ctx, *ctx_lo;                // [Mp][768]
    SeqInfo s;
    int cls_only;                      // last layer: only the query block holding <s>
};

// The one-block streaming kernel's algebra (attention_stream_kernel: S^T = K.Q^T, online base-2 softmax in fp32 with the
// reference moved only when a block's maximum leaves +-ATT_TAU, O^T += V^T.P^T, LDS images of K rows and V pieces as there)
// with three MFMAs per product, as a plain kernel: one workgroup of 4 waves = 128 query rows of one (sequence, head), grid
// (head, sequence, query part).  K and V of the whole sequence pass through a double-buffered LDS stage of 64 keys
// ((K_hi, K_lo, V_hi, V_lo) x 8 KiB = 32 KiB per stage: two workgroups per CU), loaded by all four waves whether or not their
// query rows exist; the next chunk's DMA runs under the current chunk's arithmetic.  No ring across items and no counted
// waits: attention is a tenth of the forward's flops and this mode's time goes to its GEMMs.  P is split in registers from the
// fp32 value; the row sums are those of the fp32 P.
constexpr int ATS_CHUNK = 64;
constexpr int ATS_STAGE = ATS_CHUNK * 128 * 4;   // bytes: K_hi | K_lo | V_hi | V_lo
__global__ __launch_bounds__(256, 2) void attention_split_kernel(AttnSplitArgs a) {
    constexpr float TAU = ATT_TAU;
    constexpr int PART = ATS_CHUNK * 128;        // bytes of one operand's part of a stage
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int head = blockIdx.x, b = blockIdx.y;
    const int len32 = a.s.len32[b], len = a.s.lens[b];
    const int q0 = blockIdx.z * 128;
    if (q0 >= len32) return;                     // (whole workgroup; an empty sequence has no rows at all)
    const size_t base = (size_t)a.s.off[b];
    const int r = lane & 31, hh = lane >> 5;
    const int nkb = len32 >> 5, nfull = len >> 5, nch = (len32 + ATS_CHUNK - 1) / ATS_CHUNK;
    const bool active = q0 + w * 32 < len32 && !(a.cls_only && w != 0);
    typedef const __attribute__((address_space(1))) void *gvp;
    typedef __attribute__((address_space(3))) void *lvp;

    // a chunk's 32 one-KiB pieces, 8 per wave: K pieces w and w + 4 (8 rows each; the swizzle term of piece p's rows is
    // ((p&1)*4 + (lane>>4)) & 7 and both pieces have the parity of w), V pieces w and w + 4 (16-key group p >> 1, d-tile p & 1).
    // Pieces past the sequence's last 32-key block are redirected into it (never read: no step runs on them).
    const unsigned k_lane = (unsigned)((lane >> 3) * H + ((lane & 7) ^ ((((w & 1) << 2) + (lane >> 4)) & 7)) * 8);
    const unsigned v_lane = (unsigned)((lane & 31) * 16 + (lane >> 5) * 8);
    auto issue = [&](int buf, int c) {
        unsigned char *dst = smem + buf * ATS_STAGE + w * 1024;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int p = w + 4 * j;
            const int kp = min(c * 8 + p, (len32 >> 3) - 2 + (w & 1));     // K piece of the sequence, parity kept
            const int gi = min(c * 4 + (p >> 1), (len32 >> 4) - 1);        // V group of the sequence
            const size_t ko = (base + (size_t)kp * 8) * H + head * DH + k_lane;
            const size_t vo = (((base >> 4) + gi) * H + head * DH + (p & 1) * 32) * 16 + v_lane;
            __builtin_amdgcn_global_load_lds((gvp)(a.k + ko), (lvp)(dst + j * 4096), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((gvp)(a.k_lo + ko), (lvp)(dst + PART + j * 4096), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((gvp)(a.v16 + vo), (lvp)(dst + 2 * PART + j * 4096), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((gvp)(a.v16_lo + vo), (lvp)(dst + 3 * PART + j * 4096), 16, 0, 0);
        }
    };
    issue(0, 0);
    // Q^T fragments (B operand of S^T): lane (q = r, half hh) holds q[16*ks + 8*hh .. +8)
    bf16x8 qh[4], ql[4];
    if (active) {
        const size_t qo = (base + q0 + w * 32 + r) * H + head * DH + 8 * hh;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            qh[ks] = *reinterpret_cast<const bf16x8 *>(a.q + qo + ks * 16);
            ql[ks] = *reinterpret_cast<const bf16x8 *>(a.q_lo + qo + ks * 16);
        }
    }
    const int pr = (r & 19) | ((r & 4) << 1) | ((r & 8) >> 1);  // pi(r)
    const int sw = (pr >> 1) & 7;
    auto key_of = [&](int e) { return (e & 3) + 4 * ((e >> 2) & 1) + 8 * hh + 16 * (e >> 3); };
    float m_ref = 0.f, lsum = 0.f;
    f32x16 o[2];
#pragma unroll
    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
        for (int e = 0; e < 16; ++e) o[tt][e] = 0.f;
    auto step = [&](const unsigned char *stage, int kk, int kb, auto masked_tag) {
        constexpr bool MASKED = decltype(masked_tag)::value;
        const unsigned char *kp = stage + kk * 4096 + pr * 128;
        f32x16 s;
#pragma unroll
        for (int e = 0; e < 16; ++e) s[e] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const bf16x8 kh = *reinterpret_cast<const bf16x8 *>(kp + (((2 * ks + hh) ^ sw) << 4));
            const bf16x8 kl = *reinterpret_cast<const bf16x8 *>(kp + PART + (((2 * ks + hh) ^ sw) << 4));
            s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kl, qh[ks], s, 0, 0, 0);
            s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kh, ql[ks], s, 0, 0, 0);
            s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kh, qh[ks], s, 0, 0, 0);
        }
        // scores relative to the reference; the reference starts at 0 and moves, exactly, only when it has to (the streaming
        // kernels' rule): a block's maximum more than TAU above it or -- first block -- more than TAU below
        float mloc = -INFINITY;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            s[e] -= m_ref;
            if (!MASKED || kb * 32 + key_of(e) < len) mloc = fmaxf(mloc, s[e]);
        }
        const bool first = kb == 0;
        if (__builtin_amdgcn_ballot_w64(mloc > TAU || (first && mloc < -TAU)) != 0) {   // (wave-uniform)
            const float mrow = fmaxf(mloc, __shfl_xor(mloc, 32));       // the query row's maximum over the block
            const float delta = (mrow > TAU || (first && mrow < -TAU)) ? mrow : 0.f;
            const float sc = first ? 1.f : __builtin_amdgcn_exp2f(-delta);   // (first block: l and O are still zero)
            m_ref += delta;
            lsum *= sc;
#pragma unroll
            for (int tt = 0; tt < 2; ++tt)
#pragma unroll
                for (int e = 0; e < 16; ++e) o[tt][e] *= sc;
#pragma unroll
            for (int e = 0; e < 16; ++e) s[e] -= delta;
        }
        bf16x8 ph[2], pl[2];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const bool valid = !MASKED || kb * 32 + key_of(e) < len;
            float p = valid ? __builtin_amdgcn_exp2f(s[e]) : 0.f;
            asm volatile("" : "+v"(p));
            lsum += p;
            bf16 hi, lo;
            split_bf16(p, hi, lo);
            ph[e >> 3][e & 7] = hi;
            pl[e >> 3][e & 7] = lo;
        }
        const unsigned char *vp = stage + 2 * PART + kk * 4096 + lane * 16;
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) {
                const bf16x8 vh = *reinterpret_cast<const bf16x8 *>(vp + (s2 * 2 + tt) * 1024);
                const bf16x8 vl = *reinterpret_cast<const bf16x8 *>(vp + PART + (s2 * 2 + tt) * 1024);
                o[tt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vl, ph[s2], o[tt], 0, 0, 0);
                o[tt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vh, pl[s2], o[tt], 0, 0, 0);
                o[tt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vh, ph[s2], o[tt], 0, 0, 0);
            }
    };
    __syncthreads();   // hipcc drains the LDS-DMA (vmcnt(0)) here: chunk 0 is resident
    for (int c = 0; c < nch; ++c) {
        if (c + 1 < nch) issue((c + 1) & 1, c + 1);
        if (active) {
            const unsigned char *stage = smem + (c & 1) * ATS_STAGE;
            const int kb_hi = min(nfull, (c + 1) * 2);   // blocks without padding keys
            for (int kb = c * 2; kb < kb_hi; ++kb) step(stage, kb - c * 2, kb, std::false_type{});
            if (c == nch - 1 && nfull < nkb) step(stage, nfull - c * 2, nfull, std::true_type{});
        }
        __syncthreads();   // the next chunk has landed; this stage is free
    }
    if (!active) return;
    // context rows as a pair: lane (r, hh) holds features 32t + 8g + 4hh + (0..3)
    const float inv = 1.0f / (lsum + __shfl_xor(lsum, 32));
    const size_t co = (base + q0 + w * 32 + r) * H + head * DH + 4 * hh;
#pragma unroll
    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            bf16x4 oh, ol;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float v = o[tt][g4 * 4 + j] * inv;
                asm volatile("" : "+v"(v));
                bf16 hi, lo;
                split_bf16(v, hi, lo);
                oh[j] = hi;
                ol[j] = lo;
            }
            *reinterpret_cast<bf16x4 *>(a.ctx + co + 32 * tt + 8 * g4) = oh;
            *reinterpret_cast<bf16x4 *>(a.ctx_lo + co + 32 * tt + 8 * g4) = ol;
        }
}
