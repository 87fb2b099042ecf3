// conv_pool_sb.hip — the z-free form of conv_pool.hip (first-layer Conv2D, layers.py:27-32, with the (5,4) max-pool
// window reduction of the pre-normalisation output in its epilogue) on the bf16 matrix cores: every fp32 operand is
// split exactly into three bf16 values and a product is the 6 leading partial products, accumulated in fp32 — the
// scheme of conv_sb.hip / gemm_sb.hip (fp32-level accuracy, 2.7x the rate of v_mfma_f32_32x32x2_f32).
//
// Why this layer maps well: the reduction index is k = tap * CP + channel with the channels of a pixel contiguous
// (CP = 8 slots for the 7 FOA channels, 16 for the 10 MIC ones), so the 8 consecutive k of a bf16 A fragment are ONE
// pixel's channel vector: a lane reads 16 B of the halo patch at (row + dy, bin + dx), no im2col and no transpose.
// Slot CIN of every pixel holds 1.0 and carries the bias through the centre tap's weight row; the slots above it and
// the k-steps past tap 8 meet zero weights.
//
// Tile, wave roles and the epilogue (window extreme zext, its position amax, BN statistics) are those of
// conv_first_fwd_pool_kernel<CIN, false, *>: tile = 10 image rows x 64 bins, wave = pooling row (w >> 1) x 32-bin strip
// (w & 1), 5 row tiles x 2 channel halves = 10 accumulator tiles that share the 6 weight fragments of a k-step.
// The patch (3 bf16 planes [12][66][CP]) is single-buffered: two workgroups share a CU and cover each other's staging.
//
// Two kernels: conv_first_fwd_pool_sb_kernel (4 waves, two workgroups per CU, each wave runs a tile's MFMAs and then its vector epilogue) and, for
// CIN = 7 and by default (option "conv1_pingpong"), conv_first_fwd_pool_sbpp_kernel: one 8-wave workgroup per CU whose two wave groups alternate
// matrix and vector segments across workgroup barriers, with the matrix segment software-pipelined over its LDS reads.  Same tiles per (virtual)
// workgroup in the same order, same MFMA order per accumulator: the same bits.  The schedule arithmetic is conv1_pp_sched.h.
// The vector segment runs beside the partner wave's MFMAs, where both waves' vector instructions share the 24 issue cycles an MFMA leaves free: it is
// written to the COUNT (tools/isa_mix.py, profiles/conv1_issue_budget.json): no packed fp32 (this file is built with -fno-slp-vectorize), no fmaxf.
#include "common.h"
#include "sb_tile.h"
#include "conv1_pp_sched.h"

#define CPSB_MAX_PERSISTENT 512

// v_max3_f32 by name.  fmaxf quiets every operand first (a v_max_f32 x, x per accumulator register: 160 a tile), which a maximum of MFMA results has
// no use for; beside the partner wave's MFMAs every vector instruction of the epilogue is paid in issue slots
__device__ __forceinline__ float cpsb_max3(float a, float b, float c) {
    float d;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}

template <int CIN>
struct PoolSbGeom {
    static constexpr int CP = CIN < 8 ? 8 : 16;              // channel slots per pixel (CIN values, 1.0, zeros)
    // PACK (CIN = 7, round 4): K = 64 instead of 72 (+ 8 of padding = five k-steps): the ninth tap's seven channels ride in the spare slot 7 of
    // taps 0 .. 6 (a v_perm puts element t of the tap-8 pixel's vector into the fragment of tap t), the bias in slot 7 of tap 7 (which the
    // patch already holds as 1.0): four k-steps, a fifth of the MFMAs gone
    static constexpr bool PACK = CIN == 7;
    static constexpr int KTOT = PACK ? 64 : 9 * CP;
    static constexpr int NS = (KTOT + 15) / 16;              // k-steps of 16
    // weight row stride in bf16: >= NS*16 and an odd number of 16-B slots, so the 16 lanes of a ds_read_b128 group
    // (co = lane) land on 16 different slots of the 256-B bank row
    static constexpr int KW = (((NS * 16 / 8) | 1)) * 8;
    static constexpr int PLANE = 12 * 66 * CP;               // bf16 per patch plane
    static constexpr int WPLANE = 64 * KW;
    static constexpr size_t SMEM = (size_t)(3 * PLANE + 3 * WPLANE) * 2 + 512 * sizeof(float);
};

// weights: w [9*CIN][64] fp32 (k = tap*CIN + c) -> planes [co][tap*CP + c] of the (zeroed) Wl; bias on (centre tap, slot CIN).  NT threads.
template <int CIN, bool ONE, int NT>
__device__ __forceinline__ void cpsb_stage_weights(unsigned short* Wl, const float* __restrict__ w, const float* __restrict__ bias,
                                                   const float* __restrict__ gamma, int tid) {
    using G = PoolSbGeom<CIN>;
    constexpr int CP = G::CP, KW = G::KW, WPLANE = G::WPLANE;
    for (int idx = tid; idx < (9 * CIN + 1) * 64; idx += NT) {
        const int k = idx >> 6, co = idx & 63;
        const bool isb = k == 9 * CIN;
        // output channels with gamma < 0 are computed NEGATED (weights and bias): their window extreme is then a maximum like
        // everyone else's, with no per-value sign flip in the reduction; the stored extreme and the sum are flipped back
        const float v0_ = isb ? (bias ? bias[co] : 0.f) : w[idx];
        const float v = gamma[co] < 0.f ? -v0_ : v0_;
        const int kk = G::PACK ? (isb ? 63 : (k / CIN < 8 ? (k / CIN) * CP + (k % CIN) : (k % CIN) * CP + 7))
                               : (isb ? 4 * CP + CIN : (k / CIN) * CP + (k % CIN));
        const unsigned u = __float_as_uint(v);
        const float r = v - __uint_as_float(u & 0xffff0000u);
        const unsigned vv = __float_as_uint(r);
        const float s = r - __uint_as_float(vv & 0xffff0000u);
        unsigned short* o = Wl + co * KW + kk;
        if (ONE) { o[0] = (unsigned short)bf16_rne_bits(v); continue; }
        o[0] = (unsigned short)(u >> 16);
        o[WPLANE] = (unsigned short)(vv >> 16);
        o[2 * WPLANE] = (unsigned short)(__float_as_uint(s) >> 16);
    }
}

// ONE: bf16 single-product mode (common.h KernelChoices::mfma_one): operands rounded to nearest bf16, plane 0 only, one MFMA per (k-step, row, half)
template <int CIN, bool WRITE_AMAX, bool ONE>
__global__ __launch_bounds__(256, (CIN < 8 ? 2 : 1)) void conv_first_fwd_pool_sb_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                        const float* __restrict__ bias,
                                                                        const float* __restrict__ gamma, float* __restrict__ zext,
                                                                        unsigned char* __restrict__ amax,
                                                                        float* __restrict__ stat_partial, int B, int H) {
    using G = PoolSbGeom<CIN>;
    constexpr int CP = G::CP, NS = G::NS, KW = G::KW, PLANE = G::PLANE, WPLANE = G::WPLANE;
    extern __shared__ __attribute__((aligned(16))) unsigned short cpsb_smem[];
    unsigned short* patch = cpsb_smem;                 // [3][12][66][CP]
    unsigned short* Wl = patch + 3 * PLANE;            // [3][64][KW]
    float* red = reinterpret_cast<float*>(Wl + 3 * WPLANE);   // [4][128]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kg = lane >> 5, li = lane & 31;
    const int grp = wave >> 1, strip = wave & 1;
    for (int idx = tid; idx < 3 * WPLANE / 2; idx += 256) reinterpret_cast<unsigned*>(Wl)[idx] = 0u;
    for (int idx = tid; idx < 3 * PLANE / 2; idx += 256) reinterpret_cast<unsigned*>(patch)[idx] = 0u;   // halo columns stay zero
    __syncthreads();
    cpsb_stage_weights<CIN, ONE, 256>(Wl, w, bias, gamma, tid);
    // gamma < 0: the window extreme that survives BN+ReLU+MaxPool is the minimum of z -> flip the sign, take the maximum
    const unsigned smask[2] = {gamma[li] < 0.f ? 0x80000000u : 0u, gamma[32 + li] < 0.f ? 0x80000000u : 0u};
    const int tiles_per_img = (H + 9) / 10;
    const int ntiles = B * tiles_per_img;
    const int HP = H / 5;
    // ---- patch staging: 12 rows x 64 bins = 768 pixels, 3 per thread (pixel = idx: row idx >> 6, bin idx & 63)
    float stg[3][CIN];
#define CPSB_ISSUE(tile_)                                                                               \
    {                                                                                                   \
        const int ib_ = (tile_) / tiles_per_img, it0_ = ((tile_) - ib_ * tiles_per_img) * 10;           \
        _Pragma("unroll") for (int u = 0; u < 3; ++u) {                                                 \
            const int idx = tid + 256 * u;                                                              \
            const int t = it0_ - 1 + (idx >> 6);                                                        \
            const bool ok = t >= 0 && t < H;                                                            \
            const float* p_ = ok ? x + ((size_t)(ib_ * H + t) * 64 + (idx & 63)) * CIN : x;             \
            const unsigned keep_ = ok ? 0xffffffffu : 0u;   /* AND mask: a select on a loaded value becomes a branch */ \
            _Pragma("unroll") for (int c = 0; c < CIN; ++c) stg[u][c] = __uint_as_float(__float_as_uint(p_[c]) & keep_); \
        }                                                                                               \
    }
#define CPSB_SLOT(u_, c_) ((c_) < CIN ? stg[u_][(c_) < CIN ? (c_) : 0] : ((c_) == CIN ? 1.f : 0.f))
#define CPSB_COMMIT()                                                                                   \
    _Pragma("unroll") for (int u = 0; u < 3; ++u) {                                                     \
        const int idx = tid + 256 * u;                                                                  \
        unsigned short* d_ = patch + (((idx >> 6) * 66 + (idx & 63) + 1) * CP);                         \
        _Pragma("unroll") for (int q = 0; q < CP / 8; ++q) {                                            \
            if (ONE) {                                                                                  \
                const u32x4 rv_ = {rne_pair(CPSB_SLOT(u, 8 * q + 0), CPSB_SLOT(u, 8 * q + 1)), \
                                   rne_pair(CPSB_SLOT(u, 8 * q + 2), CPSB_SLOT(u, 8 * q + 3)), \
                                   rne_pair(CPSB_SLOT(u, 8 * q + 4), CPSB_SLOT(u, 8 * q + 5)), \
                                   rne_pair(CPSB_SLOT(u, 8 * q + 6), CPSB_SLOT(u, 8 * q + 7))}; \
                *reinterpret_cast<u32x4*>(d_ + 8 * q) = rv_;                                            \
                continue;                                                                               \
            }                                                                                           \
            unsigned h0_, h1_, h2_, h3_, m0_, m1_, m2_, m3_, l0_, l1_, l2_, l3_;                        \
            split3_pair(CPSB_SLOT(u, 8 * q + 0), CPSB_SLOT(u, 8 * q + 1), h0_, m0_, l0_);          \
            split3_pair(CPSB_SLOT(u, 8 * q + 2), CPSB_SLOT(u, 8 * q + 3), h1_, m1_, l1_);          \
            split3_pair(CPSB_SLOT(u, 8 * q + 4), CPSB_SLOT(u, 8 * q + 5), h2_, m2_, l2_);          \
            split3_pair(CPSB_SLOT(u, 8 * q + 6), CPSB_SLOT(u, 8 * q + 7), h3_, m3_, l3_);          \
            const u32x4 hv_ = {h0_, h1_, h2_, h3_}, mv_ = {m0_, m1_, m2_, m3_}, lv_ = {l0_, l1_, l2_, l3_}; \
            *reinterpret_cast<u32x4*>(d_ + 8 * q) = hv_;                                                \
            *reinterpret_cast<u32x4*>(d_ + PLANE + 8 * q) = mv_;                                        \
            *reinterpret_cast<u32x4*>(d_ + 2 * PLANE + 8 * q) = lv_;                                    \
        }                                                                                               \
    }
    int tile = blockIdx.x;
    if (tile < ntiles) {
        CPSB_ISSUE(tile)
        CPSB_COMMIT()
    }
    __syncthreads();
    float s1x[2] = {0.f, 0.f}, s1y[2] = {0.f, 0.f}, s2x[2] = {0.f, 0.f}, s2y[2] = {0.f, 0.f};
    // A fragment of k-step s: lane (li, kg) reads the 8 slots [c0, c0 + 8) of pixel (row + dy, bin + dx) with
    // k0 = 16 s + 8 kg, tap = min(k0 / CP, 8) (past tap 8 the weights are zero: any finite pixel will do), c0 = k0 % CP
#define CPSB_TAP(s_, g_) ((16 * (s_) + 8 * (g_)) / CP > 8 ? 8 : (16 * (s_) + 8 * (g_)) / CP)
#define CPSB_AOFF(s_, g_) (((CPSB_TAP(s_, g_) / 3) * 66 + (CPSB_TAP(s_, g_) % 3)) * CP + ((16 * (s_) + 8 * (g_)) / CP > 8 ? 0 : (16 * (s_) + 8 * (g_)) % CP))
    const unsigned short* pbase = patch + ((5 * grp) * 66 + 32 * strip + li) * CP;
    const unsigned short* wbase = Wl + li * KW + 8 * kg;
    const int lane_e = kg * 64 + li;
    // PACK: slot 7 of the fragment <- element (2 s + kg) of the tap-8 pixel (row + 2, bin + 2): dword s of its vector, half kg
#define CPSB_FRAG(ptr_, p8_)                                                                            \
    ([&]() {                                                                                            \
        u32x4 f_ = *reinterpret_cast<const u32x4*>(ptr_);                                               \
        if (G::PACK) f_.w = __builtin_amdgcn_perm(*reinterpret_cast<const unsigned*>(p8_), f_.w, psel); \
        return __builtin_bit_cast(bf16x8, f_);                                                          \
    }())
#define CPSB_ROW(j_, ACCA_, ACCB_)                                                                      \
    {                                                                                                   \
        const unsigned short* ap_ = pa + (j_) * 66 * CP;                                                \
        const unsigned short* p8_ = p8 + (j_) * 66 * CP;                                                \
        const bf16x8 ah = CPSB_FRAG(ap_, p8_);                                                          \
        ACCA_ = mfma_bf16(ah, bh0, ACCA_); ACCB_ = mfma_bf16(ah, bh1, ACCB_);                                           \
        if (!ONE) {                                                                                     \
        const bf16x8 am = CPSB_FRAG(ap_ + PLANE, p8_ + PLANE), al = CPSB_FRAG(ap_ + 2 * PLANE, p8_ + 2 * PLANE);   \
        ACCA_ = mfma_bf16(ah, bm0, ACCA_); ACCB_ = mfma_bf16(ah, bm1, ACCB_);                                           \
        ACCA_ = mfma_bf16(am, bh0, ACCA_); ACCB_ = mfma_bf16(am, bh1, ACCB_); ACCA_ = mfma_bf16(ah, bl0, ACCA_); ACCB_ = mfma_bf16(ah, bl1, ACCB_);   \
        ACCA_ = mfma_bf16(al, bh0, ACCA_); ACCB_ = mfma_bf16(al, bh1, ACCB_); ACCA_ = mfma_bf16(am, bm0, ACCA_); ACCB_ = mfma_bf16(am, bm1, ACCB_);   \
        }                                                                                               \
    }
    // window reduction of one accumulator register of one channel half: conv_pool.hip's CP_DRAIN without the z store
#define CPSB_DRAIN(r_, c_, Y0, Y1, Y2, Y3, Y4)                                                          \
    {                                                                                                   \
        const float w0 = Y0[r_], w1 = Y1[r_], w2 = Y2[r_], w3 = Y3[r_], w4 = Y4[r_];                    \
        const float hi5 = cpsb_max3(cpsb_max3(w0, w1, w2), w3, w4);                                     \
        const bool take_ = ((r_) & 3) == 0 || hi5 > best;     /* strict: the first extreme in scan order wins ties */ \
        if (WRITE_AMAX) {    /* training: remember WHERE the extreme is: position row * 4 + column of the window */ \
            int row_ = 4;                                                                               \
            row_ = (w3 == hi5) ? 3 : row_; row_ = (w2 == hi5) ? 2 : row_;                               \
            row_ = (w1 == hi5) ? 1 : row_; row_ = (w0 == hi5) ? 0 : row_;                               \
            int pos_ = row_ * 4 + ((r_) & 3);                                                           \
            asm("" : "+v"(pos_));    /* computed for every lane: sunk under take_ it became a branch per register */ \
            bpos = take_ ? pos_ : bpos;                                                                 \
        }                                                                                               \
        best = take_ ? hi5 : best;                                                                      \
        if (((r_) & 3) == 3) {                                                                          \
            (zext + (er + (size_t)((2 * ((r_) >> 2)) * 64 + 32 * (c_))))[lane_e] = __uint_as_float(__float_as_uint(best) ^ smask[c_]); \
            if (WRITE_AMAX) (amax + (er + (size_t)((2 * ((r_) >> 2)) * 64 + 32 * (c_))))[lane_e] = (unsigned char)bpos; \
        }                                                                                               \
    }
    // BN statistics of one accumulator tile: even registers into the x accumulators, odd ones into the y accumulators (any pairing sums to the same
    // totals).  Scalar v_add_f32 / v_fma_f32 on purpose: beside MFMAs a v_pk_add_f32 / v_pk_fma_f32 costs more issue than the two it replaces
#define CPSB_STATS(c_, Y)                                                                               \
    _Pragma("unroll") for (int r = 0; r < 16; r += 2) {                                                 \
        s1x[c_] += Y[r];                                                                                \
        s2x[c_] = __builtin_fmaf(Y[r], Y[r], s2x[c_]);                                                  \
        s1y[c_] += Y[r + 1];                                                                            \
        s2y[c_] = __builtin_fmaf(Y[r + 1], Y[r + 1], s2y[c_]);                                          \
    }
    // the matrix segment of a tile: NS k-steps x 5 rows into the ten accumulator tiles accA0 .. accB4.
    // p8o: elements 2 s, 2 s + 1 of the tap-8 pixel.  The offset is laundered through an empty asm: seen as consecutive, the four k-steps' dwords
    // were merged into one ds_read_b128 per (row, plane) that stayed live for the whole tile — 60 registers, 84 spill instructions, 462 us.
    // psel: tap 7 keeps its 1.0 (the bias).  bm / bl: unused in single-product mode.
#define CPSB_TILE_MFMA()                                                                                \
    _Pragma("unroll") for (int s = 0; s < NS; ++s) {                                                    \
        const unsigned short* pa = pbase + (kg ? CPSB_AOFF(s, 1) : CPSB_AOFF(s, 0));                    \
        int p8o = 2 * s;                                                                                \
        asm volatile("" : "+s"(p8o));                                                                   \
        const unsigned short* p8 = pbase + (2 * 66 + 2) * CP + p8o;                                     \
        const unsigned psel = s == 3 ? (kg ? 0x03020100u : 0x05040100u) : (kg ? 0x07060100u : 0x05040100u); \
        const unsigned short* wp = wbase + 16 * s;                                                      \
        const bf16x8 bh0 = *reinterpret_cast<const bf16x8*>(wp), bh1 = *reinterpret_cast<const bf16x8*>(wp + 32 * KW); \
        bf16x8 bm0 = bh0, bm1 = bh1, bl0 = bh0, bl1 = bh1;                                              \
        if (!ONE) {                                                                                     \
            bm0 = *reinterpret_cast<const bf16x8*>(wp + WPLANE); bm1 = *reinterpret_cast<const bf16x8*>(wp + WPLANE + 32 * KW); \
            bl0 = *reinterpret_cast<const bf16x8*>(wp + 2 * WPLANE); bl1 = *reinterpret_cast<const bf16x8*>(wp + 2 * WPLANE + 32 * KW); \
        }                                                                                               \
        CPSB_ROW(0, accA0, accB0)                                                                       \
        CPSB_ROW(1, accA1, accB1)                                                                       \
        CPSB_ROW(2, accA2, accB2)                                                                       \
        CPSB_ROW(3, accA3, accB3)                                                                       \
        CPSB_ROW(4, accA4, accB4)                                                                       \
    }
    // the vector segment of a live pooling row: statistics, then the window extremes and their positions
#define CPSB_TILE_DRAIN()                                                                               \
    {                                                                                                   \
        CPSB_STATS(0, accA0) CPSB_STATS(0, accA1) CPSB_STATS(0, accA2) CPSB_STATS(0, accA3) CPSB_STATS(0, accA4) \
        CPSB_STATS(1, accB0) CPSB_STATS(1, accB1) CPSB_STATS(1, accB2) CPSB_STATS(1, accB3) CPSB_STATS(1, accB4) \
        _Pragma("unroll") for (int r = 0; r < 16; ++r) CPSB_DRAIN(r, 0, accA0, accA1, accA2, accA3, accA4) \
        _Pragma("unroll") for (int r = 0; r < 16; ++r) CPSB_DRAIN(r, 1, accB0, accB1, accB2, accB3, accB4) \
    }
    for (; tile < ntiles; tile += gridDim.x) {
        const int b = tile / tiles_per_img, t0 = (tile - b * tiles_per_img) * 10;
        const int nxt = tile + gridDim.x;
        CPSB_ISSUE(nxt < ntiles ? nxt : tile)
        __builtin_amdgcn_sched_barrier(0);
        const int tg = t0 + 5 * grp;             // first image row of this wave's pooling row
        const bool live = tg < H;                // H % 5 == 0: a pooling row is entirely inside or outside
        const size_t er = ((size_t)(b * HP + tg / 5) * 16 + 8 * strip) * 64;
        float best = 0.f;
        int bpos = 0;
        f32x16 accA0 = zero16(), accA1 = zero16(), accA2 = zero16(), accA3 = zero16(), accA4 = zero16();
        f32x16 accB0 = zero16(), accB1 = zero16(), accB2 = zero16(), accB3 = zero16(), accB4 = zero16();
        CPSB_TILE_MFMA()
        if (live) CPSB_TILE_DRAIN()
        // single patch buffer: everyone is done reading it, then the prefetched tile replaces it
        lds_barrier();
        CPSB_COMMIT()
        lds_barrier();
    }
    if (stat_partial) {
        float s1[2], s2[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            s1[c] = __uint_as_float(__float_as_uint(s1x[c] + s1y[c]) ^ smask[c]);     // negated channels: flip the sum back
            s2[c] = s2x[c] + s2y[c];
            s1[c] += __shfl_xor(s1[c], 32);
            s2[c] += __shfl_xor(s2[c], 32);
        }
        if (kg == 0) {
            red[wave * 128 + li] = s1[0];
            red[wave * 128 + 32 + li] = s1[1];
            red[wave * 128 + 64 + li] = s2[0];
            red[wave * 128 + 96 + li] = s2[1];
        }
        __syncthreads();
        if (tid < 128) stat_partial[(size_t)blockIdx.x * 128 + tid] = (red[tid] + red[128 + tid]) + (red[256 + tid] + red[384 + tid]);
    }
}

// ---- ping-pong form (CIN = 7; option "conv1_pingpong").  In the kernel above a wave runs a tile's 240 MFMAs and then its all-VALU epilogue, and the two
// workgroups of a CU do so in phase: both waves of a SIMD want the matrix pipe, then both leave it empty.  Here ONE 512-thread workgroup holds both: wave
// groups G0 = waves 0-3 and G1 = waves 4-7, each with the wave roles, the fragment addressing and a patch of one workgroup above, and G1 one phase behind:
//
//      barrier k:      0          1          2          3                 2 trips
//      G0         | mfma t0  | drain t0 | mfma t1  | drain t1 | ... | drain |  --   |
//      G1         |   --     | mfma t0  | drain t0 | mfma t1  | ... | mfma  | drain |
//
// so on every SIMD one wave is in its matrix segment while its partner (wave + 4) is in its vector segment.  "drain" is statistics + window extremes of
// the tile in the accumulators (which stay in registers across the barrier) and the NEXT tile's patch: its global loads are issued at the head of the
// phase (their 21 staging registers are then free during the matrix segment, which needs them for its read-ahead) and committed at its end; a patch is
// written by its own group only, in the phase after that group's reads of it.
// Group g of block b is virtual workgroup v of the kernel above's grid (conv1_pp_sched.h): the same tiles in the same order, partial row v with the same
// fold: zext, amax and the statistics partials are the same bits.  Barrier discipline: every branch around work is wave-uniform and holds NO barrier;
// all s_barrier of the loop are the four lds_barrier() below plus the two __syncthreads() of the prologue and the one of the statistics tail.
// LDS: two patches, one copy of the weight planes, red [8][128] = 105.25 KB: one workgroup per CU, two waves per SIMD as above.
template <int CIN>
struct PoolSbPpGeom {
    using G = PoolSbGeom<CIN>;
    static constexpr size_t SMEM = (size_t)(6 * G::PLANE + 3 * G::WPLANE) * 2 + 1024 * sizeof(float);
};

template <int CIN, bool WRITE_AMAX, bool ONE>
__global__ __launch_bounds__(512) void conv_first_fwd_pool_sbpp_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                        const float* __restrict__ bias, const float* __restrict__ gamma,
                                                                        float* __restrict__ zext, unsigned char* __restrict__ amax,
                                                                        float* __restrict__ stat_partial, int B, int H) {
    using G = PoolSbGeom<CIN>;
    constexpr int CP = G::CP, NS = G::NS, KW = G::KW, PLANE = G::PLANE, WPLANE = G::WPLANE;
    extern __shared__ __attribute__((aligned(16))) unsigned short cpsb_smem[];
    const int wave8 = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int pg = wave8 >> 2;                                   // wave group (scalar)
    const int tid = threadIdx.x & 255, lane = tid & 63;          // thread, wave and roles INSIDE the group: those of the 4-wave kernel
    const int wave = wave8 & 3;
    unsigned short* patch = cpsb_smem + pg * (3 * PLANE);        // [2] x [3][12][66][CP]
    unsigned short* Wl = cpsb_smem + 6 * PLANE;                  // [3][64][KW]
    float* red = reinterpret_cast<float*>(Wl + 3 * WPLANE) + pg * 512;   // [2] x [4][128]
    const int kg = lane >> 5, li = lane & 31;
    const int grp = wave >> 1, strip = wave & 1;
    for (int idx = threadIdx.x; idx < (6 * PLANE + 3 * WPLANE) / 2; idx += 512) reinterpret_cast<unsigned*>(cpsb_smem)[idx] = 0u;   // halo columns stay zero
    __syncthreads();
    cpsb_stage_weights<CIN, ONE, 512>(Wl, w, bias, gamma, threadIdx.x);
    const unsigned smask[2] = {gamma[li] < 0.f ? 0x80000000u : 0u, gamma[32 + li] < 0.f ? 0x80000000u : 0u};
    const int tiles_per_img = (H + 9) / 10;
    const int HP = H / 5;
    const Conv1PpSched sc = conv1_pp_sched(B, H);
    const int v = conv1_pp_virtual(blockIdx.x, pg);
    float stg[3][CIN];
    if (conv1_pp_active(sc, v, 0)) {
        CPSB_ISSUE(conv1_pp_tile(sc, v, 0))
        CPSB_COMMIT()
    }
    __syncthreads();
    float s1x[2] = {0.f, 0.f}, s1y[2] = {0.f, 0.f}, s2x[2] = {0.f, 0.f}, s2y[2] = {0.f, 0.f};
    const unsigned short* pbase = patch + ((5 * grp) * 66 + 32 * strip + li) * CP;
    const unsigned short* wbase = Wl + li * KW + 8 * kg;
    const int lane_e = kg * 64 + li;
    // the matrix segment, software-pipelined by one patch row: with its partner in the vector segment a wave has the matrix pipe to itself, and every
    // LDS wait in front of an MFMA is idle pipe time (with CPSB_TILE_MFMA's stream this kernel was slower than the 4-wave one, whose two workgroups
    // cover each other's waits).  Reads are issued where registers die: the high plane of row q + 1 at the head of row q, the mid plane of row q + 1
    // behind row q's eighth MFMA (the last use of its high plane), the low plane of row q at its head (eight MFMAs cover it), the next k-step's high
    // weight planes behind the last row's eighth MFMA (the last use of the low ones).  The tap-8 element is merged in (v_perm) only when a plane is
    // used, and a sched_barrier keeps each plane's wait behind the MFMAs that cover its read.  The MFMA order per accumulator is CPSB_ROW's: the same sums.
#define CPSB_RAW(s_, j_, pl_, R_, R8_, P8O_)                                                            \
    {                                                                                                   \
        const unsigned short* ap_ = pbase + (kg ? CPSB_AOFF(s_, 1) : CPSB_AOFF(s_, 0)) + (j_) * 66 * CP + (pl_) * PLANE; \
        const unsigned short* p8_ = pbase + (2 * 66 + 2 + (j_) * 66) * CP + (pl_) * PLANE + (P8O_);     \
        R_ = *reinterpret_cast<const u32x4*>(ap_); R8_ = *reinterpret_cast<const unsigned*>(p8_);       \
    }
#define CPSB_FIX(s_, R_, R8_)                                                                           \
    ([&]() {                                                                                            \
        u32x4 f_ = R_;                                                                                  \
        f_.w = __builtin_amdgcn_perm(R8_, f_.w, (s_) == 3 ? (kg ? 0x03020100u : 0x05040100u) : (kg ? 0x07060100u : 0x05040100u)); \
        return __builtin_bit_cast(bf16x8, f_);                                                          \
    }())
#define CPSB_STEP(s_, j_, has_next_, ns_, nj_, ACCA_, ACCB_, AFTER8_)                                   \
    {                                                                                                   \
        u32x4 cl = ch;                                                                                  \
        unsigned c8l = 0u;                                                                              \
        if (!ONE) CPSB_RAW(s_, j_, 2, cl, c8l, p8c)                                                     \
        if (has_next_) CPSB_RAW(ns_, nj_, 0, nh, n8h, (ns_) == (s_) ? p8c : p8n)                        \
        __builtin_amdgcn_sched_barrier(0);                                                              \
        const bf16x8 ah = CPSB_FIX(s_, ch, c8h);                                                        \
        bf16x8 am = ah;                                                                                 \
        ACCA_ = mfma_bf16(ah, bh0, ACCA_); ACCB_ = mfma_bf16(ah, bh1, ACCB_);                           \
        if (!ONE) {                                                                                     \
        ACCA_ = mfma_bf16(ah, bm0, ACCA_); ACCB_ = mfma_bf16(ah, bm1, ACCB_);                           \
        __builtin_amdgcn_sched_barrier(0);      /* a plane's wait stays behind the MFMAs that cover its read */ \
        am = CPSB_FIX(s_, cm, c8m);                                                                     \
        ACCA_ = mfma_bf16(am, bh0, ACCA_); ACCB_ = mfma_bf16(am, bh1, ACCB_); ACCA_ = mfma_bf16(ah, bl0, ACCA_); ACCB_ = mfma_bf16(ah, bl1, ACCB_);   \
        __builtin_amdgcn_sched_barrier(0);                                                              \
        if (has_next_) CPSB_RAW(ns_, nj_, 1, nm, n8m, (ns_) == (s_) ? p8c : p8n)      /* the high plane of this row is dead: room for the next row's mid plane */ \
        }                                                                                               \
        AFTER8_                                                                                         \
        __builtin_amdgcn_sched_barrier(0);                                                              \
        if (!ONE) {                                                                                     \
        const bf16x8 al = CPSB_FIX(s_, cl, c8l);                                                        \
        ACCA_ = mfma_bf16(al, bh0, ACCA_); ACCB_ = mfma_bf16(al, bh1, ACCB_); ACCA_ = mfma_bf16(am, bm0, ACCA_); ACCB_ = mfma_bf16(am, bm1, ACCB_);   \
        }                                                                                               \
        __builtin_amdgcn_sched_barrier(0);                                                              \
        ch = nh; c8h = n8h; cm = nm; c8m = n8m;                                                         \
    }
    static_assert(G::PACK, "the ping-pong form is CIN = 7's");
    if (conv1_pp_pre_barriers(pg)) lds_barrier();
    for (int it = 0; it < sc.trips; ++it) {
        const bool act = conv1_pp_active(sc, v, it);             // scalar: (block, group, iteration) alone
        const int tile = conv1_pp_tile(sc, v, it);
        const int b = tile / tiles_per_img, t0 = (tile - b * tiles_per_img) * 10;
        const int tg = t0 + 5 * grp;
        const bool live = tg < H;
        const size_t er = ((size_t)(b * HP + tg / 5) * 16 + 8 * strip) * 64;
        float best = 0.f;
        int bpos = 0;
        // set and read under act only: zeroed here, in front of the branch, they cost the matrix segment 160 v_mov per tile for the path that never reads them
        f32x16 accA0, accA1, accA2, accA3, accA4, accB0, accB1, accB2, accB3, accB4;
        if (act) {
            accA0 = accA1 = accA2 = accA3 = accA4 = accB0 = accB1 = accB2 = accB3 = accB4 = zero16();
            u32x4 ch, nh = {0u, 0u, 0u, 0u}, cm = nh, nm = nh;
            unsigned c8h, n8h = 0u, c8m = 0u, n8m = 0u;
            // offset of the tap-8 dword of k-step s (elements 2 s, 2 s + 1), laundered ONCE per k-step (see CPSB_TILE_MFMA): its fifteen reads share
            // one address register; laundered per read, each one paid an s_mov, a hazard s_nop and a v_lshl_add in the matrix wave's own gaps
            int p8c = 0;
            asm volatile("" : "+s"(p8c));
            CPSB_RAW(0, 0, 0, ch, c8h, p8c)
            if (!ONE) CPSB_RAW(0, 0, 1, cm, c8m, p8c)
            bf16x8 nbh0 = *reinterpret_cast<const bf16x8*>(wbase), nbh1 = *reinterpret_cast<const bf16x8*>(wbase + 32 * KW);
            _Pragma("unroll") for (int s = 0; s < NS; ++s) {
                const unsigned short* wp = wbase + 16 * s;
                int p8n = 2 * (s + 1);
                asm volatile("" : "+s"(p8n));
                const bf16x8 bh0 = nbh0, bh1 = nbh1;
                bf16x8 bm0 = bh0, bm1 = bh1, bl0 = bh0, bl1 = bh1;
                if (!ONE) {
                    bm0 = *reinterpret_cast<const bf16x8*>(wp + WPLANE); bm1 = *reinterpret_cast<const bf16x8*>(wp + WPLANE + 32 * KW);
                    bl0 = *reinterpret_cast<const bf16x8*>(wp + 2 * WPLANE); bl1 = *reinterpret_cast<const bf16x8*>(wp + 2 * WPLANE + 32 * KW);
                }
                CPSB_STEP(s, 0, true, s, 1, accA0, accB0, )
                CPSB_STEP(s, 1, true, s, 2, accA1, accB1, )
                CPSB_STEP(s, 2, true, s, 3, accA2, accB2, )
                CPSB_STEP(s, 3, true, s, 4, accA3, accB3, )
                // the low weight planes are dead behind the last row's eighth MFMA: room for the next k-step's high planes
                CPSB_STEP(s, 4, s + 1 < NS, s + 1, 0, accA4, accB4,
                          if (s + 1 < NS) { nbh0 = *reinterpret_cast<const bf16x8*>(wp + 16); nbh1 = *reinterpret_cast<const bf16x8*>(wp + 16 + 32 * KW); })
                p8c = p8n;
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        lds_barrier();                          // the partner group's matrix segment starts here
        __builtin_amdgcn_sched_barrier(0);
        if (act) {
            const int nxt = conv1_pp_tile(sc, v, it + 1);
            const bool more = nxt < sc.ntiles;
            if (more) CPSB_ISSUE(nxt)
            __builtin_amdgcn_sched_barrier(0);
            if (live) CPSB_TILE_DRAIN()
            if (more) CPSB_COMMIT()             // this group is done reading its patch since the barrier above
        }
        __builtin_amdgcn_sched_barrier(0);
        lds_barrier();
        __builtin_amdgcn_sched_barrier(0);
    }
    if (conv1_pp_post_barriers(pg)) lds_barrier();
    if (stat_partial) {
        float s1[2], s2[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            s1[c] = __uint_as_float(__float_as_uint(s1x[c] + s1y[c]) ^ smask[c]);
            s2[c] = s2x[c] + s2y[c];
            s1[c] += __shfl_xor(s1[c], 32);
            s2[c] += __shfl_xor(s2[c], 32);
        }
        if (kg == 0) {
            red[wave * 128 + li] = s1[0];
            red[wave * 128 + 32 + li] = s1[1];
            red[wave * 128 + 64 + li] = s2[0];
            red[wave * 128 + 96 + li] = s2[1];
        }
        __syncthreads();
        if (tid < 128 && v < sc.vgrid) stat_partial[(size_t)v * 128 + tid] = (red[tid] + red[128 + tid]) + (red[256 + tid] + red[384 + tid]);
    }
}
#undef CPSB_STEP
#undef CPSB_FIX
#undef CPSB_RAW
#undef CPSB_TILE_DRAIN
#undef CPSB_TILE_MFMA
#undef CPSB_DRAIN
#undef CPSB_STATS
#undef CPSB_ROW
#undef CPSB_FRAG
#undef CPSB_AOFF
#undef CPSB_TAP
#undef CPSB_ISSUE
#undef CPSB_COMMIT
#undef CPSB_SLOT

static int launch_cpsb_pp(hipStream_t st, const KernelChoices& kc, const float* x, const float* w, const float* bias, const float* gamma, float* zext,
                          unsigned char* amax, float* stat_partial, int* n_partial, int B, int H) {
    static_assert(CPSB_MAX_PERSISTENT == C1PP_MAX_VIRTUAL, "the ping-pong kernel plays the 4-wave kernel's grid");
    const Conv1PpSched sc = conv1_pp_sched(B, H);
    const size_t smem = PoolSbPpGeom<7>::SMEM;
#define CPSB_PP_GO(A_, ONE_)                                                                                         \
    {                                                                                                                \
        hipFuncSetAttribute(reinterpret_cast<const void*>(conv_first_fwd_pool_sbpp_kernel<7, A_, ONE_>),             \
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);                                  \
        hipLaunchKernelGGL((conv_first_fwd_pool_sbpp_kernel<7, A_, ONE_>), dim3(sc.nblocks), dim3(512), smem, st, x, w, bias, \
                           gamma, zext, amax, stat_partial, B, H);                                                   \
    }
    if (amax) { if (kc.mfma_one) CPSB_PP_GO(true, true) else CPSB_PP_GO(true, false) }
    else { if (kc.mfma_one) CPSB_PP_GO(false, true) else CPSB_PP_GO(false, false) }
#undef CPSB_PP_GO
    if (n_partial) *n_partial = sc.vgrid;
    return 0;
}

template <int CIN>
static int launch_cpsb(hipStream_t st, const KernelChoices& kc, const float* x, const float* w, const float* bias, const float* gamma, float* zext,
                       unsigned char* amax, float* stat_partial, int* n_partial, int B, int H) {
    using G = PoolSbGeom<CIN>;
    if (CIN == 7 && kc.conv1_pingpong)      // CIN = 10: two patches do not fit the LDS
        return launch_cpsb_pp(st, kc, x, w, bias, gamma, zext, amax, stat_partial, n_partial, B, H);
    const int ntiles = B * ((H + 9) / 10);
    const int grid = ntiles < CPSB_MAX_PERSISTENT ? ntiles : CPSB_MAX_PERSISTENT;
#define CPSB_GO(A_)                                                                                                 \
    {                                                                                                                \
        if (kc.mfma_one) {                                                                                           \
        hipFuncSetAttribute(reinterpret_cast<const void*>(conv_first_fwd_pool_sb_kernel<CIN, A_, true>),             \
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)G::SMEM);                               \
        hipLaunchKernelGGL((conv_first_fwd_pool_sb_kernel<CIN, A_, true>), dim3(grid), dim3(256), G::SMEM, st, x, w, bias, \
                           gamma, zext, amax, stat_partial, B, H);                                                   \
        } else {                                                                                                     \
        hipFuncSetAttribute(reinterpret_cast<const void*>(conv_first_fwd_pool_sb_kernel<CIN, A_, false>),            \
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)G::SMEM);                               \
        hipLaunchKernelGGL((conv_first_fwd_pool_sb_kernel<CIN, A_, false>), dim3(grid), dim3(256), G::SMEM, st, x, w, bias, \
                           gamma, zext, amax, stat_partial, B, H);                                                   \
        }                                                                                                            \
    }
    if (amax) CPSB_GO(true)
    else CPSB_GO(false)
#undef CPSB_GO
    if (n_partial) *n_partial = grid;
    return 0;
}

// same contract as launch_conv_first_fwd_pool with z == nullptr (conv_pool.hip)
int launch_conv_first_fwd_pool_sb(hipStream_t st, const KernelChoices& kc, const float* x, const float* w, const float* bias, const float* gamma,
                                  float* zext, unsigned char* amax, float* stat_partial, int* n_partial, int B, int H, int Cin) {
    if (H % 5 || H <= 0 || B <= 0) return -2;
    if (Cin == 7) return launch_cpsb<7>(st, kc, x, w, bias, gamma, zext, amax, stat_partial, n_partial, B, H);
    if (Cin == 10) return launch_cpsb<10>(st, kc, x, w, bias, gamma, zext, amax, stat_partial, n_partial, B, H);
    return -2;
}
