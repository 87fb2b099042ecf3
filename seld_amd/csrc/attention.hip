// attention.hip — the two operators the reference's attention blocks share (modules.transformer_encoder_block, modules.py:379-407; also the
// core of conformer_encoder_block and attention_block): multi-head scaled-dot-product self-attention over the frame axis
// (tf.keras.layers.MultiHeadAttention(n_head, key_dim)(x, x), modules.py:392-393) and LayerNormalization over the last axis (modules.py:395,
// 403), forward and backward.  C ABI "seld_attn_*" / "seld_ln_*": asynchronous on the caller's stream, no allocation, caller scratch.
//
// Attention.  Q, K, V are [B*S, H*d] row-major views with their own row strides (column slices of one fused projection need no copy);
// head h is columns h*d .. h*d+d-1.  No [B,H,S,S] tensor exists anywhere: a workgroup = 2 waves = 64 query rows (32 per wave) of one
// (batch, head) streams 64-key tiles of K and V through LDS with an online softmax (running maximum m and sum l per query row), and the
// backward recomputes the probabilities from the saved log-sum-exp m + ln l.  All products run on v_mfma_f32_32x32x2_f32 (exact fp32).
//
// Tile scheme: attn_tile.h (logits transposed, a lane owns one query in the forward and the dQ kernel and one key in the dK / dV kernel, LDS rows
// of d + 1 floats), whose steps the three kernels below are written in.  2 x 64 x 65 x 4 B = 33 KB of LDS per workgroup at d = 64 (4 workgroups
// per CU).
// Registers: Q (and dO) fragments d / 2 each, logits 16 (+16), outputs 16 ceil(d / 32) (twice that in the dK / dV kernel).
//
// Dropped probabilities (seld_attn_drop_*: tf.keras.layers.MultiHeadAttention(dropout = r), layers.MultiHeadAttention_, layers.py:253-257).
// The three kernels take the mask as a template parameter (DROP; the seld_attn_* entry points instantiate it off and stay bit-identical):
//   O[b,n,h,:] = sum_m P[n,m] M[b,h,n,m] V[b,m,h,:],  P the FULL softmax (m, l and lse see the undropped probabilities),
//   M[b,h,n,m] = 0 where u < rate, else 1 / (1 - rate);  u = (word >> 8) * 2^-24, word = word (m & 3) of
//   Philox4x32-10(counter = (m >> 2, layer, step, (b H + h) S + n), key = (seed lo, seed hi))            — attn_mask_words / attn_mask_word
// and in the backward dV_m = sum_n P M dO_n, dPd = M (dO_n . V_m), dS = P (dPd - delta), delta = rowsum(dO * O) = sum_m P M (dO . V_m): the dQ
// kernel's delta pass is the undropped one.  M is recomputed in all three kernels from that one function and never stored.  In the forward and
// dQ kernels a lane holds one query and its keys in aligned groups of four (mfma_row: (r & 3) + 8 (r >> 2) + 4 hi), so one Philox call feeds
// the four registers 4 g .. 4 g + 3.  In the dK / dV kernel the lane holds one key and 16 queries, and the four lanes of a quad hold the four keys
// of one group and the SAME 16 queries: each lane draws the words of four of them (register 4 g + (lane & 3), g = 0 .. 3) and the quad exchanges
// the keep bits by DPP — four Philox calls per 32 x 32 block and lane there too, in place of one per element.
// (b H + h) S + n must fit 32 bits: B H S <= 2^32, checked by the entry points.
//
// Any head width (seld_attnw_*: the same five entries for d in 1 .. 64).  A d that is no multiple of 8 runs the same kernels at D = 8 ceil(d / 8)
// with RAG on: the columns dd >= d are loaded as zeros and never stored (attn_tile.h), so the values are those of seld_attn_* at D on zero-padded
// operands, and the mask, which never saw D, is the same.  A multiple of 8 launches what seld_attn_* launches.
#include "attn_tile.h"

namespace {

using namespace attn_tile;

// what the DROP instantiations read (the others ignore it): the fp32 rate, 1 / (1 - rate), the Philox key and the stream
struct AttnDrop { float rate, keep; unsigned seed_lo, seed_hi, layer, step; };

// the four mask words of query element `w` = (b H + h) S + n and keys 4 m4 .. 4 m4 + 3
__device__ __forceinline__ uint4 attn_mask_words(const AttnDrop& dr, unsigned m4, unsigned w) {
    return philox4x32_10(make_uint4(m4, dr.layer, dr.step, w), make_uint2(dr.seed_lo, dr.seed_hi));
}
// lane C of every quad's value, in all four lanes of the quad
template <int C>
__device__ __forceinline__ unsigned quad_bcast(unsigned v) {
    return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, C * 0x55 /*quad_perm [C,C,C,C]*/, 0xF, 0xF, true);
}
// the keep decisions of the four keys 4 m4 .. 4 m4 + 3 for query element w, as bits 0 .. 3
__device__ __forceinline__ unsigned attn_keep_bits(const AttnDrop& dr, unsigned m4, unsigned w) {
    const uint4 r = attn_mask_words(dr, m4, w);
    return (philox_keep(r.x, dr.rate) ? 1u : 0u) | (philox_keep(r.y, dr.rate) ? 2u : 0u) | (philox_keep(r.z, dr.rate) ? 4u : 0u) |
           (philox_keep(r.w, dr.rate) ? 8u : 0u);
}

// M of the lane's 16 keys key0 + mfma_row(r, hi) (key0 a multiple of 32) of query element w: four Philox calls
__device__ __forceinline__ void attn_mask16(const AttnDrop& dr, int key0, int hi, unsigned w, float (&mk)[16]) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const uint4 r = attn_mask_words(dr, (unsigned)(key0 >> 2) + 2 * g + hi, w);
        mk[4 * g] = philox_keep(r.x, dr.rate) ? dr.keep : 0.f;
        mk[4 * g + 1] = philox_keep(r.y, dr.rate) ? dr.keep : 0.f;
        mk[4 * g + 2] = philox_keep(r.z, dr.rate) ? dr.keep : 0.f;
        mk[4 * g + 3] = philox_keep(r.w, dr.rate) ? dr.keep : 0.f;
    }
}

// Each kernel is <D, DROP, RAG>.  RAG off: the head is D columns wide (the run-time d is not read).  RAG on (seld_attnw_*): the head is d < D columns
// wide in memory, D = 8 ceil(d / 8), and the steps that touch global memory take d (attn_tile.h).  w = the head's width in memory.
template <int D, bool DROP, bool RAG>
__global__ __launch_bounds__(128) void attn_fwd_kernel(const float* __restrict__ Q, const float* __restrict__ K, const float* __restrict__ V, int ldq,
                                                       int ldk, int ldv, float* __restrict__ O, float* __restrict__ lse, int S, int H, float scale,
                                                       int nqt, AttnDrop dr, int d) {
    constexpr int LD = D + 1, NB = (D + 31) / 32;
    const int w = RAG ? d : D;
    __shared__ float Ks[ATTN_TILE * LD], Vs[ATTN_TILE * LD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 31, hi = lane >> 5;
    const int qt = blockIdx.x % nqt, bh = blockIdx.x / nqt, h = bh % H, b = bh / H;
    const int q = qt * ATTN_TILE + wave * 32 + li;
    const bool qok = q < S;
    const size_t row0 = (size_t)b * S;
    float qf[D / 2];
    load_frag<D, RAG>(Q, ldq, row0 + (qok ? q : 0), h * w, qok, hi, nullptr, scale, qf, d);
    f32x16 o[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) o[nb] = zero16();
    float m = -INFINITY, l = 0.f;
    for (int k0 = 0; k0 < S; k0 += ATTN_TILE) {
        __syncthreads();
        load_rows<D, RAG>(K, ldk, row0, k0, ATTN_TILE, S, h * w, 1.f, Ks, d);
        load_rows<D, RAG>(V, ldv, row0, k0, ATTN_TILE, S, h * w, 1.f, Vs, d);
        __syncthreads();
        for (int kb = 0; kb < 2 && k0 + kb * 32 < S; ++kb) {
            f32x16 s = logits<D>(Ks, kb * 32 + li, hi, qf);
            const float alpha = softmax_step(s, k0 + kb * 32, S, hi, m, l);
            if constexpr (DROP) {      // after the sums: l and lse are the full softmax's
                float mk[16];
                attn_mask16(dr, k0 + kb * 32, hi, (unsigned)bh * (unsigned)S + (unsigned)q, mk);
#pragma unroll
                for (int r = 0; r < 16; ++r) s[r] *= mk[r];
            }
            accum_t<D, true>(o, Vs + kb * 32 * LD, s, li, hi, alpha);
        }
    }
    store_t<D, RAG>(o, O, H * w, row0 + (qok ? q : 0), h * w, qok, hi, 1.f / l, d);
    if (lse && qok && hi == 0) lse[(size_t)bh * S + q] = m + logf(l);
}

// dQ, and delta[b][h][q] = rowsum(dO * O) for the dK / dV kernel that follows.  Same tiling as the forward.
template <int D, bool DROP, bool RAG>
__global__ __launch_bounds__(128) void attn_bwd_dq_kernel(const float* __restrict__ Q, const float* __restrict__ K, const float* __restrict__ V, int ldq,
                                                          int ldk, int ldv, const float* __restrict__ O, const float* __restrict__ dO,
                                                          const float* __restrict__ lse, float* __restrict__ dQ, int lddq, float* __restrict__ delta,
                                                          int S, int H, float scale, int nqt, AttnDrop dr, int d) {
    constexpr int LD = D + 1, NB = (D + 31) / 32;
    const int w = RAG ? d : D;
    __shared__ float Ks[ATTN_TILE * LD], Vs[ATTN_TILE * LD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 31, hi = lane >> 5;
    const int qt = blockIdx.x % nqt, bh = blockIdx.x / nqt, h = bh % H, b = bh / H;
    const int q = qt * ATTN_TILE + wave * 32 + li;
    const bool qok = q < S;
    const size_t row0 = (size_t)b * S, row = row0 + (qok ? q : 0);
    float qf[D / 2], dof[D / 2];
    load_frag<D, RAG>(Q, ldq, row, h * w, qok, hi, nullptr, scale, qf, d);
    load_frag<D, RAG>(dO, H * w, row, h * w, qok, hi, nullptr, 1.f, dof, d);
    const float dl = delta_rowsum<D, RAG>(dof, O, H * w, row, h * w, qok, hi, d);
    if (qok && hi == 0) delta[(size_t)bh * S + q] = dl;
    const float lq = qok ? lse[(size_t)bh * S + q] : INFINITY;      // a row past S: p = exp(-inf) = 0
    f32x16 dq[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) dq[nb] = zero16();
    for (int k0 = 0; k0 < S; k0 += ATTN_TILE) {
        __syncthreads();
        load_rows<D, RAG>(K, ldk, row0, k0, ATTN_TILE, S, h * w, 1.f, Ks, d);
        load_rows<D, RAG>(V, ldv, row0, k0, ATTN_TILE, S, h * w, 1.f, Vs, d);
        __syncthreads();
        for (int kb = 0; kb < 2 && k0 + kb * 32 < S; ++kb) {
            f32x16 s = logits<D>(Ks, kb * 32 + li, hi, qf);
            f32x16 dp = logits<D>(Vs, kb * 32 + li, hi, dof);
            if constexpr (DROP) {      // dPd = M (dO . V)
                float mk[16];
                attn_mask16(dr, k0 + kb * 32, hi, (unsigned)bh * (unsigned)S + (unsigned)q, mk);
#pragma unroll
                for (int r = 0; r < 16; ++r) dp[r] *= mk[r];
            }
            prob_ds_q(s, dp, k0 + kb * 32, S, hi, lq, dl);
            accum_t<D>(dq, Ks + kb * 32 * LD, s, li, hi);
        }
    }
    store_t<D, RAG>(dq, dQ, lddq, row, h * w, qok, hi, scale, d);
}

// dK and dV: a workgroup owns 64 keys of one (batch, head) (32 per wave, K and V fragments in registers) and sweeps the query tiles
template <int D, bool DROP, bool RAG>
__global__ __launch_bounds__(128) void attn_bwd_dkv_kernel(const float* __restrict__ Q, const float* __restrict__ K, const float* __restrict__ V, int ldq,
                                                           int ldk, int ldv, const float* __restrict__ dO, const float* __restrict__ lse,
                                                           const float* __restrict__ delta, float* __restrict__ dK, float* __restrict__ dV, int lddk,
                                                           int lddv, int S, int H, float scale, int nkt, AttnDrop dr, int d) {
    constexpr int LD = D + 1, NB = (D + 31) / 32;
    const int w = RAG ? d : D;
    __shared__ float Qs[ATTN_TILE * LD], Gs[ATTN_TILE * LD], ls[ATTN_TILE], ds_[ATTN_TILE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 31, hi = lane >> 5;
    const int kt = blockIdx.x % nkt, bh = blockIdx.x / nkt, h = bh % H, b = bh / H;
    const int key = kt * ATTN_TILE + wave * 32 + li;
    const bool kok = key < S;
    const size_t row0 = (size_t)b * S, row = row0 + (kok ? key : 0);
    float kf[D / 2], vf[D / 2];
    load_frag<D, RAG>(K, ldk, row, h * w, kok, hi, nullptr, 1.f, kf, d);
    load_frag<D, RAG>(V, ldv, row, h * w, kok, hi, nullptr, 1.f, vf, d);
    f32x16 dk[NB], dv[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) { dk[nb] = zero16(); dv[nb] = zero16(); }
    for (int q0 = 0; q0 < S; q0 += ATTN_TILE) {
        __syncthreads();
        load_rows<D, RAG>(Q, ldq, row0, q0, ATTN_TILE, S, h * w, scale, Qs, d);
        load_rows<D, RAG>(dO, H * w, row0, q0, ATTN_TILE, S, h * w, 1.f, Gs, d);
        load_lse_delta(lse, delta, (size_t)bh * S, q0, ATTN_TILE, S, ls, ds_);
        __syncthreads();
        for (int qb = 0; qb < 2 && q0 + qb * 32 < S; ++qb) {
            // the block's body is written out, not built from attn_tile.h's logits / accum_t: the helpers cost the DROP form 1 us of 234 at d = 24
            // and relattn.hip's twin of this kernel 11 % at d = 48; as it stands the kernel's code is the parent's, instruction for instruction
            f32x16 s = zero16(), dp = zero16();
            const float* qr = Qs + (qb * 32 + li) * LD + hi;
            const float* gr = Gs + (qb * 32 + li) * LD + hi;
#pragma unroll
            for (int st = 0; st < D / 2; ++st) s = MFMA_F32_32x32x2(qr[2 * st], kf[st], s);
#pragma unroll
            for (int st = 0; st < D / 2; ++st) dp = MFMA_F32_32x32x2(gr[2 * st], vf[st], dp);
            if constexpr (DROP) {      // dV takes P M, dS = P (M (dO . V) - delta)
#pragma unroll
                for (int r = 0; r < 16; ++r) s[r] = kok ? __expf(s[r] - ls[qb * 32 + mfma_row(r, hi)]) : 0.f;
                // the quad's lanes j = 0 .. 3 hold keys 4 m4 + j and the same 16 queries: lane j draws the words of query register 4 g + j, and
                // every lane takes bit j of the lane that drew register 4 g + c (all lanes of the wave are here: DPP)
                const int j = li & 3;
                const unsigned w0 = (unsigned)bh * (unsigned)S + (unsigned)(q0 + qb * 32);
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const unsigned bits = attn_keep_bits(dr, (unsigned)key >> 2, w0 + (unsigned)(j + 8 * g + 4 * hi));
                    const float m0 = (quad_bcast<0>(bits) >> j) & 1u ? dr.keep : 0.f, m1 = (quad_bcast<1>(bits) >> j) & 1u ? dr.keep : 0.f;
                    const float m2 = (quad_bcast<2>(bits) >> j) & 1u ? dr.keep : 0.f, m3 = (quad_bcast<3>(bits) >> j) & 1u ? dr.keep : 0.f;
                    const float* dl = ds_ + qb * 32 + 8 * g + 4 * hi;
                    dp[4 * g] = s[4 * g] * (m0 * dp[4 * g] - dl[0]);             s[4 * g] *= m0;
                    dp[4 * g + 1] = s[4 * g + 1] * (m1 * dp[4 * g + 1] - dl[1]); s[4 * g + 1] *= m1;
                    dp[4 * g + 2] = s[4 * g + 2] * (m2 * dp[4 * g + 2] - dl[2]); s[4 * g + 2] *= m2;
                    dp[4 * g + 3] = s[4 * g + 3] * (m3 * dp[4 * g + 3] - dl[3]); s[4 * g + 3] *= m3;
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int qq = qb * 32 + mfma_row(r, hi);
                    const float p = kok ? __expf(s[r] - ls[qq]) : 0.f;
                    s[r] = p;
                    dp[r] = p * (dp[r] - ds_[qq]);
                }
            }
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const int dd = nb * 32 + li;
                const bool dok = dd < D;
                const float* gc = Gs + qb * 32 * LD + (dok ? dd : 0);
                const float* qc = Qs + qb * 32 * LD + (dok ? dd : 0);
#pragma unroll
                for (int r = 0; r < 16; ++r) dv[nb] = MFMA_F32_32x32x2(dok ? gc[mfma_row(r, hi) * LD] : 0.f, s[r], dv[nb]);
#pragma unroll
                for (int r = 0; r < 16; ++r) dk[nb] = MFMA_F32_32x32x2(dok ? qc[mfma_row(r, hi) * LD] : 0.f, dp[r], dk[nb]);
            }
        }
    }
    store_t<D, RAG>(dk, dK, lddk, row, h * w, kok, hi, 1.f, d);
    store_t<D, RAG>(dv, dV, lddv, row, h * w, kok, hi, 1.f, d);
}

// ---- LayerNormalization over the last axis of [rows, C] (Keras: biased variance, eps inside the square root).  One wave per row, any C.
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// y = xhat gamma + beta, xhat = (z - mean(z)) rsqrt(var(z) + eps), z = x + r (r may be NULL); xhat / rstd saved when the pointers are given
__global__ __launch_bounds__(256) void ln_fwd_kernel(const float* __restrict__ x, const float* __restrict__ r, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, float eps, float* __restrict__ y, float* __restrict__ xhat,
                                                     float* __restrict__ rstd, int64_t rows, int C) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xp = x + row * C;
    const float* rp = r ? r + row * C : nullptr;
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += xp[c] + (rp ? rp[c] : 0.f);
    const float mean = wave_sum(s) / (float)C;
    float v = 0.f;
    for (int c = lane; c < C; c += 64) { const float t = xp[c] + (rp ? rp[c] : 0.f) - mean; v += t * t; }
    const float is = 1.f / sqrtf(wave_sum(v) / (float)C + eps);
    for (int c = lane; c < C; c += 64) {
        const float xh = (xp[c] + (rp ? rp[c] : 0.f) - mean) * is;
        if (xhat) xhat[row * C + c] = xh;
        y[row * C + c] = xh * gamma[c] + beta[c];
    }
    if (rstd && lane == 0) rstd[row] = is;
}

// dz = rstd (g - mean(g) - xhat mean(g xhat)), g = dy gamma
__global__ __launch_bounds__(256) void ln_bwd_dz_kernel(const float* __restrict__ dy, const float* __restrict__ xhat, const float* __restrict__ rstd,
                                                        const float* __restrict__ gamma, float* __restrict__ dz, int64_t rows, int C) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* dp = dy + row * C;
    const float* hp = xhat + row * C;
    float a = 0.f, b = 0.f;
    for (int c = lane; c < C; c += 64) { const float g = dp[c] * gamma[c]; a += g; b += g * hp[c]; }
    const float ma = wave_sum(a) / (float)C, mb = wave_sum(b) / (float)C, is = rstd[row];
    for (int c = lane; c < C; c += 64) dz[row * C + c] = is * (dp[c] * gamma[c] - ma - hp[c] * mb);
}

// dgamma = sum_rows dy xhat, dbeta = sum_rows dy in two stages: workgroup (bx, by) sums a contiguous run of rows of the columns by * 256 + t
// (coalesced rows, double accumulators) into part[bx][2][C]; then one thread per column adds the partials in workgroup order
#define LN_MAX_BLOCKS 256
__global__ __launch_bounds__(256) void ln_bwd_partial_kernel(const float* __restrict__ dy, const float* __restrict__ xhat, float* __restrict__ part,
                                                             int64_t rows, int C) {
    const int c = blockIdx.y * 256 + threadIdx.x;
    if (c >= C) return;
    const int64_t per = (rows + gridDim.x - 1) / gridDim.x, p0 = (int64_t)blockIdx.x * per, p1 = p0 + per < rows ? p0 + per : rows;
    double a = 0.0, b = 0.0;
    for (int64_t p = p0; p < p1; ++p) { const double d = dy[p * C + c]; a += d; b += d * (double)xhat[p * C + c]; }
    part[(size_t)blockIdx.x * 2 * C + c] = (float)a;
    part[(size_t)blockIdx.x * 2 * C + C + c] = (float)b;
}
__global__ __launch_bounds__(256) void ln_bwd_fold_kernel(const float* __restrict__ part, int nb, int C, float* __restrict__ dgamma,
                                                          float* __restrict__ dbeta) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double a = 0.0, b = 0.0;
    for (int k = 0; k < nb; ++k) { a += part[(size_t)k * 2 * C + c]; b += part[(size_t)k * 2 * C + C + c]; }
    dbeta[c] = (float)a;
    dgamma[c] = (float)b;
}
inline int ln_blocks(int64_t rows) { const int64_t b = (rows + 15) / 16; return (int)(b < LN_MAX_BLOCKS ? b : LN_MAX_BLOCKS); }

// launch `kern`<D_, drop, rag> on `grid` workgroups (static LDS)
#define AT_LAUNCH(D_, kern, drop, rag, grid, st, ...) hipLaunchKernelGGL((kern<D_, drop, rag>), dim3(grid), dim3(128), 0, st, __VA_ARGS__)
#define AT_DISPATCH(kern, drop, d, grid, st, ...) ATTN_DISPATCH_D(d, AT_LAUNCH, kern, drop, false, grid, st, __VA_ARGS__, d)
// the ragged form: `kern`<8 ceil(d / 8), drop, true>
#define ATW_DISPATCH(kern, drop, d, grid, st, ...) ATTN_DISPATCH_D(((d) + 7) & ~7, AT_LAUNCH, kern, drop, true, grid, st, __VA_ARGS__, d)

inline bool rate_ok(float rate) { return rate >= 0.f && rate < 1.f; }      // (a NaN fails both)
// the mask counter's last word (b H + h) S + n is 32 bits wide
inline bool ctr_ok(int B, int S, int H) { return (int64_t)B * H * S <= ((int64_t)1 << 32); }      // B * H fits an int behind tile_grid: no overflow
inline AttnDrop at_drop(float rate, uint64_t seed, unsigned layer, unsigned step) {
    return AttnDrop{rate, 1.f / (1.f - rate), (unsigned)seed, (unsigned)(seed >> 32), layer, step};
}

// seld_attn_fwd (rate 0: the mask-free instantiations, whatever seed / layer / step) and seld_attn_drop_fwd; any_d: seld_attnw_* — d in 1..64,
// a multiple of 8 launches what seld_attn_* launches and any other d the ragged kernels
int attn_fwd_impl(bool any_d, const float* Q, const float* K, const float* V, int ldq, int ldk, int ldv, float* O, float* lse, int B, int S, int H, int d,
                  float scale, float rate, uint64_t seed, unsigned layer, unsigned step, void* stream) {
    if (!(any_d ? dw_ok(d) : d_ok(d))) return SELD_ERR_UNSUPPORTED;
    if (!Q || !K || !V || !O || B < 1 || S < 1 || H < 1 || !ld_ok(ldq, H, d) || !ld_ok(ldk, H, d) || !ld_ok(ldv, H, d) || !rate_ok(rate))
        return SELD_ERR_INVALID;
    const int64_t grid = tile_grid(B, S, H);
    if (grid < 0) return SELD_ERR_UNSUPPORTED;
    const int nt = (int)(grid / B / H);
    const AttnDrop dr = at_drop(rate, seed, layer, step);
    const bool rag = d % 8 != 0;
    if (rate > 0.f) {
        if (!ctr_ok(B, S, H)) return SELD_ERR_UNSUPPORTED;
        if (rag) {
            ATW_DISPATCH(attn_fwd_kernel, true, d, (unsigned)grid, (hipStream_t)stream, Q, K, V, ldq, ldk, ldv, O, lse, S, H, scale, nt, dr);
        } else {
            AT_DISPATCH(attn_fwd_kernel, true, d, (unsigned)grid, (hipStream_t)stream, Q, K, V, ldq, ldk, ldv, O, lse, S, H, scale, nt, dr);
        }
    } else if (rag) {
        ATW_DISPATCH(attn_fwd_kernel, false, d, (unsigned)grid, (hipStream_t)stream, Q, K, V, ldq, ldk, ldv, O, lse, S, H, scale, nt, dr);
    } else {
        AT_DISPATCH(attn_fwd_kernel, false, d, (unsigned)grid, (hipStream_t)stream, Q, K, V, ldq, ldk, ldv, O, lse, S, H, scale, nt, dr);
    }
    return ok();
}

int attn_bwd_impl(bool any_d, const float* Q, const float* K, const float* V, int ldq, int ldk, int ldv, const float* O, const float* dO, const float* lse,
                  float* dQ, float* dK, float* dV, int lddq, int lddk, int lddv, float* scratch, int B, int S, int H, int d, float scale,
                  float rate, uint64_t seed, unsigned layer, unsigned step, void* stream) {
    if (!(any_d ? dw_ok(d) : d_ok(d))) return SELD_ERR_UNSUPPORTED;
    if (!Q || !K || !V || !O || !dO || !lse || !dQ || !dK || !dV || !scratch || B < 1 || S < 1 || H < 1 || !ld_ok(ldq, H, d) || !ld_ok(ldk, H, d) ||
        !ld_ok(ldv, H, d) || !ld_ok(lddq, H, d) || !ld_ok(lddk, H, d) || !ld_ok(lddv, H, d) || !rate_ok(rate))
        return SELD_ERR_INVALID;
    const int64_t grid = tile_grid(B, S, H);
    if (grid < 0) return SELD_ERR_UNSUPPORTED;
    const int nt = (int)(grid / B / H);
    const AttnDrop dr = at_drop(rate, seed, layer, step);
    const bool rag = d % 8 != 0;
    if (rate > 0.f) {
        if (!ctr_ok(B, S, H)) return SELD_ERR_UNSUPPORTED;
        if (rag) {
            ATW_DISPATCH(attn_bwd_dq_kernel, true, d, (unsigned)grid, (hipStream_t)stream, Q, K, V, ldq, ldk, ldv, O, dO, lse, dQ, lddq, scratch, S, H,
                         scale, nt, dr);
            ATW_DISPATCH(attn_bwd_dkv_kernel, true, d, (unsigned)grid, (hipStream_t)stream, Q, K, V, ldq, ldk, ldv, dO, lse, scratch, dK, dV, lddk, lddv, S,
                         H, scale, nt, dr);
            return ok();
        }
        AT_DISPATCH(attn_bwd_dq_kernel, true, d, (unsigned)grid, (hipStream_t)stream, Q, K, V, ldq, ldk, ldv, O, dO, lse, dQ, lddq, scratch, S, H, scale,
                    nt, dr);
        AT_DISPATCH(attn_bwd_dkv_kernel, true, d, (unsigned)grid, (hipStream_t)stream, Q, K, V, ldq, ldk, ldv, dO, lse, scratch, dK, dV, lddk, lddv, S, H,
                    scale, nt, dr);
    } else if (rag) {
        ATW_DISPATCH(attn_bwd_dq_kernel, false, d, (unsigned)grid, (hipStream_t)stream, Q, K, V, ldq, ldk, ldv, O, dO, lse, dQ, lddq, scratch, S, H,
                     scale, nt, dr);
        ATW_DISPATCH(attn_bwd_dkv_kernel, false, d, (unsigned)grid, (hipStream_t)stream, Q, K, V, ldq, ldk, ldv, dO, lse, scratch, dK, dV, lddk, lddv, S,
                     H, scale, nt, dr);
    } else {
        AT_DISPATCH(attn_bwd_dq_kernel, false, d, (unsigned)grid, (hipStream_t)stream, Q, K, V, ldq, ldk, ldv, O, dO, lse, dQ, lddq, scratch, S, H, scale,
                    nt, dr);
        AT_DISPATCH(attn_bwd_dkv_kernel, false, d, (unsigned)grid, (hipStream_t)stream, Q, K, V, ldq, ldk, ldv, dO, lse, scratch, dK, dV, lddk, lddv, S, H,
                    scale, nt, dr);
    }
    return ok();
}

}  // namespace

extern "C" {

int seld_attn_fwd(const float* Q, const float* K, const float* V, int ldq, int ldk, int ldv, float* O, float* lse, int B, int S, int H, int d,
                  float scale, void* stream) {
    return attn_fwd_impl(false, Q, K, V, ldq, ldk, ldv, O, lse, B, S, H, d, scale, 0.f, 0, 0, 0, stream);
}

/* floats of caller scratch seld_attn_bwd takes: delta[b][h][q] = rowsum(dO * O) */
int64_t seld_attn_bwd_scratch(int B, int S, int H, int d) {
    if (!d_ok(d) || B < 1 || S < 1 || H < 1 || (int64_t)H * d > 0x7fffffff || tile_grid(B, S, H) < 0) return -1;      // what seld_attn_bwd refuses
    return (int64_t)B * H * S;      // B * H fits an int here: no overflow
}

int seld_attn_bwd(const float* Q, const float* K, const float* V, int ldq, int ldk, int ldv, const float* O, const float* dO, const float* lse,
                  float* dQ, float* dK, float* dV, int lddq, int lddk, int lddv, float* scratch, int B, int S, int H, int d, float scale,
                  void* stream) {
    return attn_bwd_impl(false, Q, K, V, ldq, ldk, ldv, O, dO, lse, dQ, dK, dV, lddq, lddk, lddv, scratch, B, S, H, d, scale, 0.f, 0, 0, 0, stream);
}

/* the same with the probabilities dropped (header comment): rate 0 launches exactly what seld_attn_fwd / _bwd launch */
int seld_attn_drop_fwd(const float* Q, const float* K, const float* V, int ldq, int ldk, int ldv, float* O, float* lse, int B, int S, int H, int d,
                       float scale, float rate, uint64_t seed, unsigned layer, unsigned step, void* stream) {
    return attn_fwd_impl(false, Q, K, V, ldq, ldk, ldv, O, lse, B, S, H, d, scale, rate, seed, layer, step, stream);
}

int seld_attn_drop_bwd(const float* Q, const float* K, const float* V, int ldq, int ldk, int ldv, const float* O, const float* dO, const float* lse,
                       float* dQ, float* dK, float* dV, int lddq, int lddk, int lddv, float* scratch, int B, int S, int H, int d, float scale,
                       float rate, uint64_t seed, unsigned layer, unsigned step, void* stream) {
    return attn_bwd_impl(false, Q, K, V, ldq, ldk, ldv, O, dO, lse, dQ, dK, dV, lddq, lddk, lddv, scratch, B, S, H, d, scale, rate, seed, layer, step,
                         stream);
}

/* seld_attnw_*: the five entries above for any head width d in 1..64 (header comment of attn_tile.h); a multiple of 8 launches what they launch */
int seld_attnw_fwd(const float* Q, const float* K, const float* V, int ldq, int ldk, int ldv, float* O, float* lse, int B, int S, int H, int d,
                   float scale, void* stream) {
    return attn_fwd_impl(true, Q, K, V, ldq, ldk, ldv, O, lse, B, S, H, d, scale, 0.f, 0, 0, 0, stream);
}

int64_t seld_attnw_bwd_scratch(int B, int S, int H, int d) {
    if (!dw_ok(d) || B < 1 || S < 1 || H < 1 || (int64_t)H * d > 0x7fffffff || tile_grid(B, S, H) < 0) return -1;      // what seld_attnw_bwd refuses
    return (int64_t)B * H * S;
}

int seld_attnw_bwd(const float* Q, const float* K, const float* V, int ldq, int ldk, int ldv, const float* O, const float* dO, const float* lse,
                   float* dQ, float* dK, float* dV, int lddq, int lddk, int lddv, float* scratch, int B, int S, int H, int d, float scale,
                   void* stream) {
    return attn_bwd_impl(true, Q, K, V, ldq, ldk, ldv, O, dO, lse, dQ, dK, dV, lddq, lddk, lddv, scratch, B, S, H, d, scale, 0.f, 0, 0, 0, stream);
}

int seld_attnw_drop_fwd(const float* Q, const float* K, const float* V, int ldq, int ldk, int ldv, float* O, float* lse, int B, int S, int H, int d,
                        float scale, float rate, uint64_t seed, unsigned layer, unsigned step, void* stream) {
    return attn_fwd_impl(true, Q, K, V, ldq, ldk, ldv, O, lse, B, S, H, d, scale, rate, seed, layer, step, stream);
}

int seld_attnw_drop_bwd(const float* Q, const float* K, const float* V, int ldq, int ldk, int ldv, const float* O, const float* dO, const float* lse,
                        float* dQ, float* dK, float* dV, int lddq, int lddk, int lddv, float* scratch, int B, int S, int H, int d, float scale,
                        float rate, uint64_t seed, unsigned layer, unsigned step, void* stream) {
    return attn_bwd_impl(true, Q, K, V, ldq, ldk, ldv, O, dO, lse, dQ, dK, dV, lddq, lddk, lddv, scratch, B, S, H, d, scale, rate, seed, layer, step,
                         stream);
}

int seld_ln_fwd(const float* x, const float* r, const float* gamma, const float* beta, float eps, float* y, float* xhat, float* rstd, int64_t rows,
                int C, void* stream) {
    if (!x || !gamma || !beta || !y || rows < 1 || C < 1 || (rows + 3) / 4 > 0x7fffffff) return SELD_ERR_INVALID;
    hipLaunchKernelGGL(ln_fwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, r, gamma, beta, eps, y, xhat, rstd, rows, C);
    return ok();
}

/* floats of caller scratch seld_ln_bwd takes: the first-stage partial sums of dgamma / dbeta, [workgroups <= 256][2][C] */
int64_t seld_ln_scratch(int64_t rows, int C) { return rows > 0 && C > 0 ? (int64_t)ln_blocks(rows) * 2 * C : -1; }

int seld_ln_bwd(const float* dy, const float* xhat, const float* rstd, const float* gamma, float* dz, float* dgamma, float* dbeta, float* scratch,
                int64_t rows, int C, void* stream) {
    if (!dy || !xhat || !rstd || !gamma || !dz || !dgamma || !dbeta || !scratch || rows < 1 || C < 1 || (rows + 3) / 4 > 0x7fffffff)
        return SELD_ERR_INVALID;
    const int nb = ln_blocks(rows);
    hipLaunchKernelGGL(ln_bwd_partial_kernel, dim3(nb, (C + 255) / 256), dim3(256), 0, (hipStream_t)stream, dy, xhat, scratch, rows, C);
    hipLaunchKernelGGL(ln_bwd_fold_kernel, dim3((C + 255) / 256), dim3(256), 0, (hipStream_t)stream, scratch, nb, C, dgamma, dbeta);
    hipLaunchKernelGGL(ln_bwd_dz_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, dy, xhat, rstd, gamma, dz, rows, C);
    return ok();
}

}  // extern "C"
