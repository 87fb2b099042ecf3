// relattn.hip — the reference's layers.RelPositionMultiHeadAttention core (layers.py:332-392), the attention of modules.attention_block with
// abs_pos_encoding = False (modules.py:585-588), forward and backward, and attention_block's stand-alone GLU (modules.py:598-601).  C ABI
// "seld_relattn_*" / "seld_glu_*": asynchronous on the caller's stream, no allocation, caller scratch.
//
//   logit[i,j] = scale (qu_i . k_j + shifted[i,j]),  qu = q + u, qv = q + vb,  G[i,m] = qv_i . P_m,  shifted = relative_shift(G)
//
// relative_shift (pad one zero column in front, reshape [S, S+1] -> [S+1, S], drop the first row) is an index map.  With P' the table P
// followed by one zero row (index S) and c = S - 1 - i + j:
//   shifted[i,j] = qv_i . P'[c]                 for j <= i   (c <= S - 1)
//                = qv_{i+1} . P'[c - S - 1]     for j >  i   (c = S is the zero row: the j = i + 1 diagonal; the NEXT query row otherwise)
// so along a query row the table index runs with j - i only: a 64-query x 64-key tile needs the 127 consecutive rows c0 .. c0 + 126 of the
// band B[c] = P'[c mod (S + 1)], and the product of a 32-query block with 64 band rows, read back along the skewed diagonal, is the
// positional term of a 32 x 32 logit block.  Blocks below the diagonal take it from qv_i, blocks above from qv_{i+1}, the diagonal block both.
//
// Forward and the dQ kernel keep attention.hip's tile scheme (attn_tile.h: a lane owns one query, logits transposed, online softmax); the band product
// Gt[band row][query] goes through a per-wave LDS tile [64][32] and is read back at row (key - query + 31): both the write (lanes = queries of
// one row) and the skewed read (row stride 32, lane stride -31 .. the addresses of a half-wave are 32 different banks) are conflict-free.  The
// backward of the shift is the same map run backwards: dS of a block is scattered to band rows and contracted with the band on the MFMA.
//   relattn_bwd_dq   dQu (own rows), the j <= i part of dQv (own rows), the j >= i + 2 part, which belongs to row i + 1, to scratch
//   relattn_bwd_dkv  dK, dV: a lane owns one key; G[query][band] through LDS [32][64], read at column (key - query + 31)
//   relattn_bwd_dp   dP: a lane owns one table row m.  m fixes j - i (m - S + 1 below the diagonal, m + 2 above), so a workgroup of 64 rows m
//                    walks the two diagonal stripes that read them: the content logits and dO . V of a 32-query block against a 96-key band
//                    are skewed through LDS, the positional term needs no skew there.  Per-batch partials go to scratch.
//   relattn_fold     dQv[i] += the scratch row i - 1;  dP = the batches' partials added in batch order
// Every output element is owned by one lane or folded in a fixed order: no atomics, two runs give the same bits.  No [B,H,S,S] (nor S x (S+1))
// tensor exists; scratch is B H S (1 + 2 d) floats.  All products run on v_mfma_f32_32x32x2_f32 (exact fp32).
#include "attn_tile.h"

namespace {

using namespace attn_tile;

// orders a wave's own LDS writes and reads of its private tile (LDS operations of one wave complete in order; the compiler must not move them)
__device__ __forceinline__ void wave_lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// the lane index again, opaque to the optimiser: the per-register lane masks of the skewed reads are then compared where they are used (one
// v_cmp each) instead of being hoisted out of the tile loop into 32 - 48 mask pairs that no scalar register file holds
__device__ __forceinline__ int opaque(int v) { asm volatile("" : "+v"(v)); return v; }

// band rows c0 .. c0 + n - 1 of one head: B[c] = P[c] (c < S), 0 (c = S), P[c - S - 1] (S < c <= 2 S), 0 elsewhere -> LDS [n][D + 1]
template <int D>
__device__ __forceinline__ void load_band(const float* __restrict__ P, int ldp, int col0, int S, int64_t c0, int n, float* dst) {
    for (int e = threadIdx.x; e < n * D; e += 128) {
        const int t = e / D, dd = e - t * D;
        const int64_t c = c0 + t;
        const int64_t m = c < S ? c : c - S - 1;
        dst[t * (D + 1) + dd] = c >= 0 && c != S && c <= 2 * (int64_t)S ? P[(size_t)m * ldp + col0 + dd] : 0.f;
    }
}

// Gt[band row][query] of the wave's 32 queries (rows qrow .. of an LDS tile, lane li's row given) against 64 band rows -> Gw [64][32]
template <int D>
__device__ __forceinline__ void band_t(const float* pb, const float* qrow, float* Gw, int li, int hi) {
    constexpr int LD = D + 1;
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
        f32x16 g = zero16();
        const float* pr = pb + (blk * 32 + li) * LD + hi;
#pragma unroll
        for (int st = 0; st < D / 2; ++st) g = MFMA_F32_32x32x2(pr[2 * st], qrow[2 * st], g);
#pragma unroll
        for (int r = 0; r < 16; ++r) Gw[(blk * 32 + mfma_row(r, hi)) * 32 + li] = g[r];
    }
}

// s[key][query] += the positional term of the block (keys J0 .. J0 + 31, the wave's queries I0 .. I0 + 31; both multiples of 32)
template <int D>
__device__ __forceinline__ void add_positional_t(f32x16& s, const float* pb, const float* Qv, float* Gw, int I0, int J0, int wave, int li, int hi) {
    constexpr int LD = D + 1;
    if (J0 <= I0) {      // j <= i: this query's row
        wave_lds_sync();
        band_t<D>(pb, Qv + (wave * 32 + li) * LD + hi, Gw, li, hi);
        wave_lds_sync();
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int jj = mfma_row(r, hi);
            const float v = Gw[(jj - li + 31) * 32 + li];
            if (J0 < I0 || jj <= opaque(li)) s[r] += v;
        }
    }
    if (J0 >= I0) {      // j > i: the next query's row (the band's zero row at j = i + 1)
        wave_lds_sync();
        band_t<D>(pb, Qv + (wave * 32 + li + 1) * LD + hi, Gw, li, hi);
        wave_lds_sync();
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int jj = mfma_row(r, hi);
            const float v = Gw[(jj - li + 31) * 32 + li];
            if (J0 > I0 || jj > opaque(li)) s[r] += v;
        }
    }
}

template <int D>
constexpr int ra_lds_qtile() { return ((2 * ATTN_TILE + 2 * ATTN_TILE + ATTN_TILE + 1) * (D + 1) + 2 * 64 * 32) * (int)sizeof(float); }

// Workgroup = 64 queries of one (batch, head); LDS: K, V tiles [64][D+1], band [128][D+1], qv rows I0w .. I0w + 64 [65][D+1], Gw [2][64][32]
template <int D>
__global__ __launch_bounds__(128) void relattn_fwd_kernel(const float* __restrict__ Q, const float* __restrict__ K, const float* __restrict__ V, int ldq,
                                                          int ldk, int ldv, const float* __restrict__ P, int ldp, const float* __restrict__ u,
                                                          const float* __restrict__ vb, float* __restrict__ O, float* __restrict__ lse, int S, int H,
                                                          float scale, int nqt) {
    constexpr int LD = D + 1, NB = (D + 31) / 32;
    extern __shared__ float sm[];
    float* Ks = sm;
    float* Vs = Ks + ATTN_TILE * LD;
    float* Pb = Vs + ATTN_TILE * LD;
    float* Qv = Pb + 2 * ATTN_TILE * LD;
    float* Gs = Qv + (ATTN_TILE + 1) * LD;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), li = lane & 31, hi = lane >> 5;
    const int qt = blockIdx.x % nqt, bh = blockIdx.x / nqt, h = bh % H, b = bh / H;
    const int I0w = qt * ATTN_TILE, I0 = I0w + wave * 32, q = I0 + li;
    const bool qok = q < S;
    const size_t row0 = (size_t)b * S;
    float* Gw = Gs + wave * 64 * 32;
    float qf[D / 2];
    load_frag<D>(Q, ldq, row0 + (qok ? q : 0), h * D, qok, hi, u, scale, qf);
    load_rows<D>(Q, ldq, row0, I0w, ATTN_TILE + 1, S, h * D, vb, scale, Qv);
    f32x16 o[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) o[nb] = zero16();
    float m = -INFINITY, l = 0.f;
    for (int k0 = 0; k0 < S; k0 += ATTN_TILE) {
        __syncthreads();
        load_rows<D>(K, ldk, row0, k0, ATTN_TILE, S, h * D, 1.f, Ks);
        load_rows<D>(V, ldv, row0, k0, ATTN_TILE, S, h * D, 1.f, Vs);
        load_band<D>(P, ldp, h * D, S, (int64_t)S - 1 + k0 - I0w - 63, 2 * ATTN_TILE, Pb);
        __syncthreads();
        for (int kb = 0; kb < 2 && k0 + kb * 32 < S; ++kb) {
            f32x16 s = logits<D>(Ks, kb * 32 + li, hi, qf);
            add_positional_t<D>(s, Pb + (kb * 32 - wave * 32 + 32) * LD, Qv, Gw, I0, k0 + kb * 32, wave, li, hi);
            const float alpha = softmax_step(s, k0 + kb * 32, S, hi, m, l);
            accum_t<D, true>(o, Vs + kb * 32 * LD, s, li, hi, alpha);
        }
    }
    store_t<D>(o, O, H * D, row0 + (qok ? q : 0), h * D, qok, hi, 1.f / l);
    if (lse && qok && hi == 0) lse[(size_t)bh * S + q] = m + logf(l);
}

// acc^T[dd][query] += sum over the block's keys of band[c(query, key)][dd] ds[key][query], the keys masked by `lower` (j <= i) or not (j > i)
template <int D>
__device__ __forceinline__ void scatter_band_t(f32x16 (&acc)[(D + 31) / 32], const f32x16& ds, const float* pb, float* Gw, bool lower, int I0, int J0,
                                               int li, int hi) {
    constexpr int LD = D + 1, NB = (D + 31) / 32;
    wave_lds_sync();
    const int lv = opaque(li);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int jj = mfma_row(r, hi);
        const bool keep = lower ? (J0 < I0 || jj <= lv) : (J0 > I0 || jj > lv);
        Gw[(jj - li + 31) * 32 + li] = keep ? ds[r] : 0.f;
    }
    wave_lds_sync();
#pragma unroll
    for (int blk = 0; blk < 2; ++blk)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int mm = blk * 32 + mfma_row(r, hi);
            const float gv = Gw[mm * 32 + li];
            const float dg = (unsigned)(mm + lv - 31) < 32u ? gv : 0.f;      // the 32 band rows this query's keys reach
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const int dd = nb * 32 + li;
                const bool dok = dd < D;
                acc[nb] = MFMA_F32_32x32x2(dok ? pb[mm * LD + dd] : 0.f, dg, acc[nb]);
            }
        }
}

// dQu, the j <= i part of dQv, the j > i part (row i + 1's) to `dqv_next`, and delta[b][h][q] = rowsum(dO * O).  Same tiling as the forward.
template <int D>
__global__ __launch_bounds__(128) void relattn_bwd_dq_kernel(const float* __restrict__ Q, const float* __restrict__ K, const float* __restrict__ V,
                                                             int ldq, int ldk, int ldv, const float* __restrict__ P, int ldp,
                                                             const float* __restrict__ u, const float* __restrict__ vb, const float* __restrict__ O,
                                                             const float* __restrict__ dO, const float* __restrict__ lse, float* __restrict__ dQu,
                                                             float* __restrict__ dQv, int lddqu, int lddqv, float* __restrict__ delta,
                                                             float* __restrict__ dqv_next, int S, int H, float scale, int nqt) {
    constexpr int LD = D + 1, NB = (D + 31) / 32;
    extern __shared__ float sm[];
    float* Ks = sm;
    float* Vs = Ks + ATTN_TILE * LD;
    float* Pb = Vs + ATTN_TILE * LD;
    float* Qv = Pb + 2 * ATTN_TILE * LD;
    float* Gs = Qv + (ATTN_TILE + 1) * LD;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), li = lane & 31, hi = lane >> 5;
    const int qt = blockIdx.x % nqt, bh = blockIdx.x / nqt, h = bh % H, b = bh / H;
    const int I0w = qt * ATTN_TILE, I0 = I0w + wave * 32, q = I0 + li;
    const bool qok = q < S;
    const size_t row0 = (size_t)b * S, row = row0 + (qok ? q : 0);
    float* Gw = Gs + wave * 64 * 32;
    float qf[D / 2], dof[D / 2];
    load_frag<D>(Q, ldq, row, h * D, qok, hi, u, scale, qf);
    load_frag<D>(dO, H * D, row, h * D, qok, hi, nullptr, 1.f, dof);
    load_rows<D>(Q, ldq, row0, I0w, ATTN_TILE + 1, S, h * D, vb, scale, Qv);
    const float dl = delta_rowsum<D>(dof, O, H * D, row, h * D, qok, hi);
    if (qok && hi == 0) delta[(size_t)bh * S + q] = dl;
    const float lq = qok ? lse[(size_t)bh * S + q] : INFINITY;      // a row past S: p = exp(-inf) = 0
    f32x16 dqu[NB], dqa[NB], dqb[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) { dqu[nb] = zero16(); dqa[nb] = zero16(); dqb[nb] = zero16(); }
    for (int k0 = 0; k0 < S; k0 += ATTN_TILE) {
        __syncthreads();
        load_rows<D>(K, ldk, row0, k0, ATTN_TILE, S, h * D, 1.f, Ks);
        load_rows<D>(V, ldv, row0, k0, ATTN_TILE, S, h * D, 1.f, Vs);
        load_band<D>(P, ldp, h * D, S, (int64_t)S - 1 + k0 - I0w - 63, 2 * ATTN_TILE, Pb);
        __syncthreads();
        for (int kb = 0; kb < 2 && k0 + kb * 32 < S; ++kb) {
            const int J0 = k0 + kb * 32;
            const float* pb = Pb + (kb * 32 - wave * 32 + 32) * LD;
            f32x16 s = logits<D>(Ks, kb * 32 + li, hi, qf);
            add_positional_t<D>(s, pb, Qv, Gw, I0, J0, wave, li, hi);
            const f32x16 dp = logits<D>(Vs, kb * 32 + li, hi, dof);
            prob_ds_q(s, dp, J0, S, hi, lq, dl);
            // attn_tile.h's accum_t, spelled out: through the helper the d >= 32 instantiations of this kernel and of relattn_bwd_dp_kernel pair one
            // more couple of LDS reads into a ds_read2_b32 — the same words, but not the parent's instruction counts
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const int dd = nb * 32 + li;
                const bool dok = dd < D;
                const float* kc = Ks + kb * 32 * LD + (dok ? dd : 0);
#pragma unroll
                for (int r = 0; r < 16; ++r) dqu[nb] = MFMA_F32_32x32x2(dok ? kc[mfma_row(r, hi) * LD] : 0.f, s[r], dqu[nb]);
            }
            if (J0 <= I0) scatter_band_t<D>(dqa, s, pb, Gw, true, I0, J0, li, hi);
            if (J0 >= I0) scatter_band_t<D>(dqb, s, pb, Gw, false, I0, J0, li, hi);
        }
    }
    store_t<D>(dqu, dQu, lddqu, row, h * D, qok, hi, scale);
    store_t<D>(dqa, dQv, lddqv, row, h * D, qok, hi, scale);
    store_t<D>(dqb, dqv_next, H * D, row, h * D, qok, hi, scale);
}

template <int D>
constexpr int ra_lds_ktile() { return ((ATTN_TILE + ATTN_TILE + 1 + ATTN_TILE + 2 * ATTN_TILE) * (D + 1) + 2 * ATTN_TILE + 2 * 32 * 64) * (int)sizeof(float); }

// dK and dV: a workgroup owns 64 keys of one (batch, head) (32 per wave, K and V fragments in registers) and sweeps the query tiles.
// LDS: qu [64][D+1], qv rows q0 .. q0 + 64 [65][D+1], dO [64][D+1], band [128][D+1], lse / delta [64] each, Gw [2][32][64]
template <int D>
__global__ __launch_bounds__(128) void relattn_bwd_dkv_kernel(const float* __restrict__ Q, const float* __restrict__ K, const float* __restrict__ V,
                                                              int ldq, int ldk, int ldv, const float* __restrict__ P, int ldp,
                                                              const float* __restrict__ u, const float* __restrict__ vb,
                                                              const float* __restrict__ dO, const float* __restrict__ lse,
                                                              const float* __restrict__ delta, float* __restrict__ dK, float* __restrict__ dV, int lddk,
                                                              int lddv, int S, int H, float scale, int nkt) {
    constexpr int LD = D + 1, NB = (D + 31) / 32;
    extern __shared__ float sm[];
    float* Qu = sm;
    float* Qv = Qu + ATTN_TILE * LD;
    float* Gd = Qv + (ATTN_TILE + 1) * LD;
    float* Pb = Gd + ATTN_TILE * LD;
    float* ls = Pb + 2 * ATTN_TILE * LD;
    float* ds_ = ls + ATTN_TILE;
    float* Gs = ds_ + ATTN_TILE;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), li = lane & 31, hi = lane >> 5;
    const int kt = blockIdx.x % nkt, bh = blockIdx.x / nkt, h = bh % H, b = bh / H;
    const int J0w = kt * ATTN_TILE, J0 = J0w + wave * 32, key = J0 + li;
    const bool kok = key < S;
    const size_t row0 = (size_t)b * S, row = row0 + (kok ? key : 0);
    float* Gw = Gs + wave * 32 * 64;
    float kf[D / 2], vf[D / 2];
    load_frag<D>(K, ldk, row, h * D, kok, hi, nullptr, 1.f, kf);
    load_frag<D>(V, ldv, row, h * D, kok, hi, nullptr, 1.f, vf);
    f32x16 dk[NB], dv[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) { dk[nb] = zero16(); dv[nb] = zero16(); }
    for (int q0 = 0; q0 < S; q0 += ATTN_TILE) {
        __syncthreads();
        load_rows<D>(Q, ldq, row0, q0, ATTN_TILE, S, h * D, u, scale, Qu);
        load_rows<D>(Q, ldq, row0, q0, ATTN_TILE + 1, S, h * D, vb, scale, Qv);
        load_rows<D>(dO, H * D, row0, q0, ATTN_TILE, S, h * D, 1.f, Gd);
        load_band<D>(P, ldp, h * D, S, (int64_t)S - 1 + J0w - q0 - 63, 2 * ATTN_TILE, Pb);
        load_lse_delta(lse, delta, (size_t)bh * S, q0, ATTN_TILE, S, ls, ds_);
        __syncthreads();
        for (int qb = 0; qb < 2 && q0 + qb * 32 < S; ++qb) {
            const int I0 = q0 + qb * 32;
            const float* pb = Pb + (wave * 32 - qb * 32 + 32) * LD;
            // from here to the accumulations the parent's own text, not attn_tile.h's logits / accum_t: through the helpers this kernel ran 11 %
            // slower at d = 48 (695 -> 774 us)
            f32x16 s = zero16(), dp = zero16();
            const float* qr = Qu + (qb * 32 + li) * LD + hi;
            const float* gr = Gd + (qb * 32 + li) * LD + hi;
#pragma unroll
            for (int st = 0; st < D / 2; ++st) s = MFMA_F32_32x32x2(qr[2 * st], kf[st], s);
            // the positional term: G[query][band column] of the block through Gw [32][64], read at column key - query + 31
#pragma unroll
            for (int up = 0; up < 2; ++up) {
                if (up ? J0 < I0 : J0 > I0) continue;
                const float* ar = Qv + (qb * 32 + li + up) * LD + hi;
                wave_lds_sync();
#pragma unroll
                for (int blk = 0; blk < 2; ++blk) {
                    f32x16 g = zero16();
                    const float* br = pb + (blk * 32 + li) * LD + hi;
#pragma unroll
                    for (int st = 0; st < D / 2; ++st) g = MFMA_F32_32x32x2(ar[2 * st], br[2 * st], g);
#pragma unroll
                    for (int r = 0; r < 16; ++r) Gw[mfma_row(r, hi) * 64 + blk * 32 + li] = g[r];
                }
                wave_lds_sync();
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int ii = mfma_row(r, hi);
                    const float v = Gw[ii * 64 + li - ii + 31];
                    const int lv = opaque(li);
                    if (up ? (J0 > I0 || lv > ii) : (J0 < I0 || lv <= ii)) s[r] += v;
                }
            }
#pragma unroll
            for (int st = 0; st < D / 2; ++st) dp = MFMA_F32_32x32x2(gr[2 * st], vf[st], dp);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int qq = qb * 32 + mfma_row(r, hi);
                const float p = kok ? __expf(s[r] - ls[qq]) : 0.f;
                s[r] = p;
                dp[r] = p * (dp[r] - ds_[qq]);
            }
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const int dd = nb * 32 + li;
                const bool dok = dd < D;
                const float* gc = Gd + qb * 32 * LD + (dok ? dd : 0);
                const float* qc = Qu + qb * 32 * LD + (dok ? dd : 0);
#pragma unroll
                for (int r = 0; r < 16; ++r) dv[nb] = MFMA_F32_32x32x2(dok ? gc[mfma_row(r, hi) * LD] : 0.f, s[r], dv[nb]);
#pragma unroll
                for (int r = 0; r < 16; ++r) dk[nb] = MFMA_F32_32x32x2(dok ? qc[mfma_row(r, hi) * LD] : 0.f, dp[r], dk[nb]);
            }
        }
    }
    store_t<D>(dk, dK, lddk, row, h * D, kok, hi, 1.f);      // qu carries the scale
    store_t<D>(dv, dV, lddv, row, h * D, kok, hi, 1.f);
}

template <int D>
constexpr int ra_lds_ptile() { return ((96 + 96 + 32 + 33 + 32) * (D + 1) + 64 + 2 * 32 * 64) * (int)sizeof(float); }

// x[query][key window column kk] of a 32-query block against the wave's 64 key-band rows, read back at column (query + lane): the stripe's key
template <int D>
__device__ __forceinline__ f32x16 stripe_product(const float* arow, const float* band, float* Gw, int li, int hi) {
    constexpr int LD = D + 1;
    wave_lds_sync();
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
        f32x16 g = zero16();
        const float* br = band + (blk * 32 + li) * LD + hi;
#pragma unroll
        for (int st = 0; st < D / 2; ++st) g = MFMA_F32_32x32x2(arow[2 * st], br[2 * st], g);
#pragma unroll
        for (int r = 0; r < 16; ++r) Gw[mfma_row(r, hi) * 64 + blk * 32 + li] = g[r];
    }
    wave_lds_sync();
    f32x16 out;
#pragma unroll
    for (int r = 0; r < 16; ++r) { const int ii = mfma_row(r, hi); out[r] = Gw[ii * 64 + ii + li]; }
    return out;
}

// dP partial of one batch: a workgroup owns 64 table rows m of one (batch, head) and walks the query blocks twice — the stripe j = i + m - S + 1
// (j <= i, weighs qv_i) and the stripe j = i + m + 2 (j >= i + 2, weighs qv_{i+1}).
// LDS: K, V bands [96][D+1], qu [32][D+1], qv rows I0 .. I0 + 32 [33][D+1], dO [32][D+1], lse / delta [32] each, Gw [2][32][64]
template <int D>
__global__ __launch_bounds__(128) void relattn_bwd_dp_kernel(const float* __restrict__ Q, const float* __restrict__ K, const float* __restrict__ V,
                                                             int ldq, int ldk, int ldv, const float* __restrict__ P, int ldp,
                                                             const float* __restrict__ u, const float* __restrict__ vb, const float* __restrict__ dO,
                                                             const float* __restrict__ lse, const float* __restrict__ delta,
                                                             float* __restrict__ part, int S, int H, float scale, int nmt) {
    constexpr int LD = D + 1, NB = (D + 31) / 32;
    extern __shared__ float sm[];
    float* Kb = sm;
    float* Vb = Kb + 96 * LD;
    float* Qu = Vb + 96 * LD;
    float* Qv = Qu + 32 * LD;
    float* Gd = Qv + 33 * LD;
    float* ls = Gd + 32 * LD;
    float* ds_ = ls + 32;
    float* Gs = ds_ + 32;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), li = lane & 31, hi = lane >> 5;
    const int mt = blockIdx.x % nmt, bh = blockIdx.x / nmt, h = bh % H, b = bh / H;
    const int M0w = mt * ATTN_TILE, m = M0w + wave * 32 + li;
    const bool mok = m < S;
    const size_t row0 = (size_t)b * S;
    float* Gw = Gs + wave * 32 * 64;
    float pf[D / 2];
    load_frag<D>(P, ldp, (size_t)(mok ? m : 0), h * D, mok, hi, nullptr, 1.f, pf);
    f32x16 acc[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[nb] = zero16();
    for (int up = 0; up < 2; ++up) {
        const int64_t d0 = up ? (int64_t)M0w + 2 : (int64_t)M0w - S + 1;      // j - i of the workgroup's first row m
        const int64_t dm = d0 + wave * 32 + li;
        for (int I0 = 0; I0 < S; I0 += 32) {
            if (I0 + d0 > S - 1 || I0 + 31 + d0 + 63 < 0) continue;      // the stripe's keys of this block lie outside [0, S)
            __syncthreads();
            load_rows<D>(K, ldk, row0, (int)(I0 + d0), 96, S, h * D, 1.f, Kb);
            load_rows<D>(V, ldv, row0, (int)(I0 + d0), 96, S, h * D, 1.f, Vb);
            load_rows<D>(Q, ldq, row0, I0, 32, S, h * D, u, scale, Qu);
            load_rows<D>(Q, ldq, row0, I0, 33, S, h * D, vb, scale, Qv);
            load_rows<D>(dO, H * D, row0, I0, 32, S, h * D, 1.f, Gd);
            load_lse_delta(lse, delta, (size_t)bh * S, I0, 32, S, ls, ds_);
            __syncthreads();
            f32x16 s = stripe_product<D>(Qu + li * LD + hi, Kb + wave * 32 * LD, Gw, li, hi);
            f32x16 dp = stripe_product<D>(Gd + li * LD + hi, Vb + wave * 32 * LD, Gw, li, hi);
            s += logits<D>(Qv, li + up, hi, pf);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ii = mfma_row(r, hi);
                const int64_t j = I0 + ii + dm;
                const float p = mok && j >= 0 && j < S ? __expf(s[r] - ls[ii]) : 0.f;      // (a query past S: lse = inf)
                s[r] = p * (dp[r] - ds_[ii]);
            }
            // accum_t spelled out: see relattn_bwd_dq_kernel
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const int dd = nb * 32 + li;
                const bool dok = dd < D;
                const float* qc = Qv + up * LD + (dok ? dd : 0);
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[nb] = MFMA_F32_32x32x2(dok ? qc[mfma_row(r, hi) * LD] : 0.f, s[r], acc[nb]);
            }
        }
    }
    store_t<D>(acc, part, H * D, row0 + (mok ? m : 0), h * D, mok, hi, 1.f);      // qv carries the scale
}

// dQv[b, s, :] += next[b, s - 1, :] (s >= 1);  dP[m, :] = sum_b part[b, m, :] in batch order
__global__ __launch_bounds__(256) void relattn_fold_kernel(float* __restrict__ dQv, int lddqv, const float* __restrict__ next, float* __restrict__ dP,
                                                           int lddp, const float* __restrict__ part, int B, int S, int HD, int64_t nq, int64_t np) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < nq) {
        const int64_t row = e / HD;
        const int c = (int)(e - row * HD);
        if (row % S) dQv[row * lddqv + c] += next[(row - 1) * HD + c];
    } else if (e - nq < np) {
        const int64_t f = e - nq, m = f / HD;
        const int c = (int)(f - m * HD);
        float a = 0.f;
        for (int b = 0; b < B; ++b) a += part[((int64_t)b * S + m) * HD + c];
        dP[m * lddp + c] = a;
    }
}

// y = u[:, :C] * sigmoid(u[:, C:])
__global__ __launch_bounds__(256) void glu_fwd_kernel(const float* __restrict__ u, int64_t ldu, float* __restrict__ y, int64_t n, int C) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const int64_t r = e / C;
    const int c = (int)(e - r * C);
    const float a = u[r * ldu + c], g = u[r * ldu + C + c];
    const float ex = expf(-fabsf(g)), rr = 1.f / (1.f + ex);
    y[e] = a * (g >= 0.f ? rr : ex * rr);
}
// du[:, :C] = dy sigmoid(b), du[:, C:] = dy a sigmoid'(b); the derivative without cancellation or overflow at any b: e = exp(-|b|) <= 1
__global__ __launch_bounds__(256) void glu_bwd_kernel(const float* __restrict__ u, int64_t ldu, const float* __restrict__ dy, float* __restrict__ du,
                                                      int64_t lddu, int64_t n, int C) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const int64_t r = e / C;
    const int c = (int)(e - r * C);
    const float a = u[r * ldu + c], g = u[r * ldu + C + c];
    const float ex = expf(-fabsf(g)), rr = 1.f / (1.f + ex);
    du[r * lddu + c] = dy[e] * (g >= 0.f ? rr : ex * rr);
    du[r * lddu + C + c] = dy[e] * a * (ex * rr * rr);
}

// attn_tile.h's grid, or -1 also where a band index 2 S leaves an int
inline int64_t ra_grid(int B, int S, int H) { return S > 0x3fffff00 ? -1 : tile_grid(B, S, H); }

// launch `kern`<D_> with `ldsfn`<D_>() bytes of dynamic LDS
#define RA_LAUNCH(D_, kern, ldsfn, grid, st, ...)                                                                            \
    {                                                                                                                        \
        if (ldsfn<D_>() > 65536)                                                                                             \
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern<D_>), hipFuncAttributeMaxDynamicSharedMemorySize, ldsfn<D_>()); \
        hipLaunchKernelGGL((kern<D_>), dim3(grid), dim3(128), ldsfn<D_>(), st, __VA_ARGS__);                                 \
    }
#define RA_DISPATCH(kern, ldsfn, d, grid, st, ...) ATTN_DISPATCH_D(d, RA_LAUNCH, kern, ldsfn, grid, st, __VA_ARGS__)

}  // namespace

extern "C" {

int seld_relattn_fwd(const float* Q, const float* K, const float* V, int ldq, int ldk, int ldv, const float* P, int ldp, const float* u,
                     const float* vb, float* O, float* lse, int B, int S, int H, int d, float scale, void* stream) {
    if (!d_ok(d)) return SELD_ERR_UNSUPPORTED;
    if (!Q || !K || !V || !P || !u || !vb || !O || B < 1 || S < 1 || H < 1 || !ld_ok(ldq, H, d) || !ld_ok(ldk, H, d) || !ld_ok(ldv, H, d) ||
        !ld_ok(ldp, H, d))
        return SELD_ERR_INVALID;
    const int64_t grid = ra_grid(B, S, H);
    if (grid < 0) return SELD_ERR_UNSUPPORTED;
    const int nt = (int)(grid / B / H);
    RA_DISPATCH(relattn_fwd_kernel, ra_lds_qtile, d, (unsigned)grid, (hipStream_t)stream, Q, K, V, ldq, ldk, ldv, P, ldp, u, vb, O, lse, S, H, scale, nt);
    return ok();
}

/* floats of caller scratch seld_relattn_bwd takes: delta [B, H, S], the j > i part of dQv [B*S, H*d], the batches' dP partials [B*S, H*d] */
int64_t seld_relattn_bwd_scratch(int B, int S, int H, int d) {
    if (!d_ok(d) || B < 1 || S < 1 || H < 1 || (int64_t)H * d > 0x7fffffff || ra_grid(B, S, H) < 0) return -1;      // what seld_relattn_bwd refuses
    return (int64_t)B * H * S * (1 + 2 * d);      // B * H * ceil(S / 64) fits an int here: no overflow
}

int seld_relattn_bwd(const float* Q, const float* K, const float* V, int ldq, int ldk, int ldv, const float* P, int ldp, const float* u,
                     const float* vb, const float* O, const float* dO, const float* lse, float* dQu, float* dQv, float* dK, float* dV, float* dP,
                     int lddqu, int lddqv, int lddk, int lddv, int lddp, float* scratch, int B, int S, int H, int d, float scale, void* stream) {
    if (!d_ok(d)) return SELD_ERR_UNSUPPORTED;
    if (!Q || !K || !V || !P || !u || !vb || !O || !dO || !lse || !dQu || !dQv || !dK || !dV || !dP || !scratch || B < 1 || S < 1 || H < 1 ||
        !ld_ok(ldq, H, d) || !ld_ok(ldk, H, d) || !ld_ok(ldv, H, d) || !ld_ok(ldp, H, d) || !ld_ok(lddqu, H, d) || !ld_ok(lddqv, H, d) ||
        !ld_ok(lddk, H, d) || !ld_ok(lddv, H, d) || !ld_ok(lddp, H, d))
        return SELD_ERR_INVALID;
    const int64_t grid = ra_grid(B, S, H);
    if (grid < 0) return SELD_ERR_UNSUPPORTED;
    const int nt = (int)(grid / B / H), HD = H * d;
    const int64_t nq = (int64_t)B * S * HD, np = (int64_t)S * HD;
    if ((nq + np + 255) / 256 > 0x7fffffff) return SELD_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    float* delta = scratch;
    float* next = delta + (int64_t)B * H * S;
    float* part = next + nq;
    RA_DISPATCH(relattn_bwd_dq_kernel, ra_lds_qtile, d, (unsigned)grid, st, Q, K, V, ldq, ldk, ldv, P, ldp, u, vb, O, dO, lse, dQu, dQv, lddqu, lddqv,
                delta, next, S, H, scale, nt);
    RA_DISPATCH(relattn_bwd_dkv_kernel, ra_lds_ktile, d, (unsigned)grid, st, Q, K, V, ldq, ldk, ldv, P, ldp, u, vb, dO, lse, delta, dK, dV, lddk, lddv,
                S, H, scale, nt);
    RA_DISPATCH(relattn_bwd_dp_kernel, ra_lds_ptile, d, (unsigned)grid, st, Q, K, V, ldq, ldk, ldv, P, ldp, u, vb, dO, lse, delta, part, S, H, scale,
                nt);
    hipLaunchKernelGGL(relattn_fold_kernel, dim3((unsigned)((nq + np + 255) / 256)), dim3(256), 0, st, dQv, lddqv, next, dP, lddp, part, B, S, HD, nq,
                       np);
    return ok();
}

int seld_glu_fwd(const float* u, int ldu, float* y, int64_t rows, int C, void* stream) {
    if (!u || !y || rows < 1 || C < 1 || (int64_t)ldu < 2 * (int64_t)C) return SELD_ERR_INVALID;
    if (rows > 0x7fffffffffffLL / C || (rows * C + 255) / 256 > 0x7fffffff) return SELD_ERR_UNSUPPORTED;
    const int64_t n = rows * C;
    hipLaunchKernelGGL(glu_fwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, u, (int64_t)ldu, y, n, C);
    return ok();
}

int seld_glu_bwd(const float* u, int ldu, const float* dy, float* du, int lddu, int64_t rows, int C, void* stream) {
    if (!u || !dy || !du || rows < 1 || C < 1 || (int64_t)ldu < 2 * (int64_t)C || (int64_t)lddu < 2 * (int64_t)C) return SELD_ERR_INVALID;
    if (rows > 0x7fffffffffffLL / C || (rows * C + 255) / 256 > 0x7fffffff) return SELD_ERR_UNSUPPORTED;
    const int64_t n = rows * C;
    hipLaunchKernelGGL(glu_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, u, (int64_t)ldu, dy, du, (int64_t)lddu, n,
                       C);
    return ok();
}

}  // extern "C"
