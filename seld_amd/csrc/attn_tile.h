// attn_tile.h — the tile steps the flash-style attention kernels are written in: attention.hip (attn_fwd / attn_bwd_dq / attn_bwd_dkv) and
// relattn.hip (relattn_fwd / relattn_bwd_dq / relattn_bwd_dkv / relattn_bwd_dp), and the host checks and the launch dispatch of both.
// Private to this directory.
//
// Tile scheme (forward, and the dQ kernels of the backward): the logits are computed TRANSPOSED, S^T[key][query] = K Q^T, so that a lane
// of the accumulator layout (common.h) holds ONE query (column l & 31) and 16 keys (rows (r & 3) + 8 (r >> 2) + 4 (l >> 5)); lane l ^ 32
// holds the other 16.  The row maximum and sum of a query are then 16 in-lane operations and one cross-half shuffle, m / l / lse / delta are
// per-lane scalars, and the accumulator registers p[r] ARE the B operand of the next product O^T[dd][query] += V^T[dd][key] P^T[key][query]
// (step r contracts keys row(r, 0) and row(r, 1): a sum over keys has no order to respect), so P never crosses LDS.  The dK / dV kernels are
// the mirror image: S[query][key] with the key on the lane and K, V of the wave's 32 keys in registers, Q and dO tiles through LDS, and
// p[r] / ds[r] the B operands of dV^T += dO^T P and dK^T += Q^T dS.  Each output element is owned by exactly one lane of one workgroup:
// no atomics, sums in a fixed order, two runs are bit-identical.
//
// LDS rows are d + 1 floats (odd): the [key = lane][dd] operand reads of a 32-lane half then hit 32 different banks, and the
// [key = row][dd = lane] reads are consecutive addresses.
//
// In every function: li = lane & 31, hi = lane >> 5; a workgroup is 128 threads (two waves of 32 rows each).
//
// Ragged head widths (RAG, seld_attnw_* of attention.hip): a head of d columns, d no multiple of 8, runs the D = 8 ceil(d / 8) instantiation with
// the run-time d in the steps that touch global memory — load_frag and load_rows put zeros in columns dd >= d, store_t skips them, delta_rowsum
// reads only real columns.  The LDS tiles, the fragments and every MFMA chain keep their D columns: a zero column adds exact zeros, so the values
// are those of the D-wide kernel on zero-padded operands.  RAG is a template parameter (default off) for the reason BIAS is one below: the
// instantiations without it keep their code, instruction for instruction.  Single dwords move, so nothing beyond 4-byte alignment is assumed.
#pragma once
#include "common.h"
#include <math.h>

#define ATTN_TILE 64      // query rows per workgroup = keys per LDS tile (two 32-row MFMA blocks)

namespace attn_tile {

__device__ __forceinline__ float xhalf(float v) { return __shfl_xor(v, 32, 64); }

// the lane's fragment of row `row` (valid: ok) of a view: f[s] = (row[2 s + hi] + bias[2 s + hi]) * mul; bias may be NULL
template <int D, bool RAG = false>
__device__ __forceinline__ void load_frag(const float* __restrict__ src, int ld, size_t row, int col0, bool ok, int hi, const float* __restrict__ bias,
                                          float mul, float (&f)[D / 2], int d = D) {
    const float* p = src + row * (size_t)ld + col0 + hi;
#pragma unroll
    for (int s = 0; s < D / 2; ++s) {
        float v = 0.f;
        if (ok && (!RAG || 2 * s + hi < d)) {
            v = p[2 * s];
            if (bias) v += bias[col0 + hi + 2 * s];
            v *= mul;
        }
        f[s] = v;
    }
}

// out^T[dd][lane's row] accumulators -> out[row][col0 + dd] * mul
template <int D, bool RAG = false>
__device__ __forceinline__ void store_t(const f32x16 (&acc)[(D + 31) / 32], float* __restrict__ out, int ld, size_t row, int col0, bool ok, int hi,
                                        float mul, int d = D) {
    if (!ok) return;
    float* p = out + row * (size_t)ld + col0;
#pragma unroll
    for (int nb = 0; nb < (D + 31) / 32; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int dd = nb * 32 + mfma_row(r, hi);
            if (dd < D && (!RAG || dd < d)) p[dd] = acc[nb][r] * mul;
        }
}

// rows r0 .. r0 + n - 1 of one head of a [B*S, ld] view (BIAS: + bias[col0 + dd]; then * mul, the query's 1 / sqrt(key_dim)) -> LDS [n][D + 1];
// rows outside [0, S) as zeros.  Called through the two load_rows overloads below.  BIAS is a template parameter, not a NULL test: a run-time
// `if (bias)` inside this loop changed the code of half the attention.hip kernels, this form leaves the loader's users as they were
template <int D, bool BIAS, bool RAG>
__device__ __forceinline__ void load_rows_impl(const float* __restrict__ src, int ld, size_t row0, int r0, int n, int S, int col0,
                                               const float* __restrict__ bias, float mul, float* dst, int d) {
    for (int e = threadIdx.x; e < n * D; e += 128) {
        const int rr = e / D, dd = e - rr * D;
        const int r = r0 + rr;
        float v = 0.f;
        if (r >= 0 && r < S && (!RAG || dd < d)) {
            v = src[(row0 + r) * (size_t)ld + col0 + dd];
            if constexpr (BIAS) v += bias[col0 + dd];
            v *= mul;
        }
        dst[rr * (D + 1) + dd] = v;
    }
}
template <int D, bool RAG = false>
__device__ __forceinline__ void load_rows(const float* __restrict__ src, int ld, size_t row0, int r0, int n, int S, int col0, float mul, float* dst,
                                          int d = D) {
    load_rows_impl<D, false, RAG>(src, ld, row0, r0, n, S, col0, nullptr, mul, dst, d);
}
template <int D, bool RAG = false>      // with a bias (not NULL)
__device__ __forceinline__ void load_rows(const float* __restrict__ src, int ld, size_t row0, int r0, int n, int S, int col0,
                                          const float* __restrict__ bias, float mul, float* dst, int d = D) {
    load_rows_impl<D, true, RAG>(src, ld, row0, r0, n, S, col0, bias, mul, dst, d);
}

// lse / delta of queries q0 .. q0 + n - 1 of one (batch, head) (base = its first element) -> LDS; a row past S gets lse = inf: p = exp(-inf) = 0
__device__ __forceinline__ void load_lse_delta(const float* __restrict__ lse, const float* __restrict__ delta, size_t base, int q0, int n, int S,
                                               float* ls, float* ds) {
    if ((int)threadIdx.x < n) {
        const int q = q0 + threadIdx.x;
        ls[threadIdx.x] = q < S ? lse[base + q] : INFINITY;
        ds[threadIdx.x] = q < S ? delta[base + q] : 0.f;
    }
}

// the logits product: acc[r][lane's column] = sum_dd tile[row][dd] frag[dd], row = the lane's row of the LDS tile [.][D + 1], D / 2 MFMA steps
template <int D>
__device__ __forceinline__ f32x16 logits(const float* tile, int row, int hi, const float (&frag)[D / 2]) {
    const float* t = tile + row * (D + 1) + hi;
    f32x16 acc = zero16();
#pragma unroll
    for (int st = 0; st < D / 2; ++st) acc = MFMA_F32_32x32x2(t[2 * st], frag[st], acc);
    return acc;
}

// one 32-key block (keys key0 + mfma_row(r, hi), key0 < S) of the online softmax of the lane's query: masks the keys past S, updates the running
// maximum m and sum l, turns the logits s into exp(s - m) and returns alpha = exp(old m - m), the rescale of what was accumulated so far
__device__ __forceinline__ float softmax_step(f32x16& s, int key0, int S, int hi, float& m, float& l) {
    float mx = m;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        if (key0 + mfma_row(r, hi) >= S) s[r] = -INFINITY;      // the edge tile's keys past S
        mx = fmaxf(mx, s[r]);
    }
    mx = fmaxf(mx, xhalf(mx));      // finite: the block's first key is < S
    const float alpha = __expf(m - mx);
    float ps = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) { s[r] = __expf(s[r] - mx); ps += s[r]; }
    ps += xhalf(ps);
    l = l * alpha + ps;
    m = mx;
    return alpha;
}

// the transposed accumulation of one 32-column block nb: acc^T[dd][lane] += sum_r rows[mfma_row(r, hi)][dd] w[r], dd = 32 nb + li; rows = 32 rows
// of an LDS tile [.][D + 1], w the lane's 16 weights (p or ds); the lanes dd >= D of the last block feed zeros.  By value: with acc and w by
// reference attn_bwd_dkv_kernel<56, true> took 260 registers for 256 and lost its second wave per SIMD
template <int D>
__device__ __forceinline__ f32x16 accum_block(f32x16 acc, const float* rows, int nb, f32x16 w, int li, int hi) {
    const int dd = nb * 32 + li;
    const bool dok = dd < D;
    const float* c = rows + (dok ? dd : 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) acc = MFMA_F32_32x32x2(dok ? c[mfma_row(r, hi) * (D + 1)] : 0.f, w[r], acc);
    return acc;
}
// ... of all ceil(D / 32) blocks; RESCALE: acc *= alpha first (the forward's running output under a new maximum)
template <int D, bool RESCALE = false>
__device__ __forceinline__ void accum_t(f32x16 (&acc)[(D + 31) / 32], const float* rows, const f32x16& w, int li, int hi, float alpha = 1.f) {
#pragma unroll
    for (int nb = 0; nb < (D + 31) / 32; ++nb) {
        if constexpr (RESCALE) {
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[nb][r] *= alpha;
        }
        acc[nb] = accum_block<D>(acc[nb], rows, nb, w, li, hi);
    }
}

// the dQ kernels' prologue: delta = rowsum(dO * O) of the lane's row (valid: ok) from its dO fragment; the caller writes it to the scratch
template <int D, bool RAG = false>
__device__ __forceinline__ float delta_rowsum(const float (&dof)[D / 2], const float* __restrict__ O, int ld, size_t row, int col0, bool ok, int hi,
                                              int d = D) {
    const float* op = O + row * (size_t)ld + col0 + hi;
    float dl = 0.f;
#pragma unroll
    for (int s = 0; s < D / 2; ++s) dl += ok && (!RAG || 2 * s + hi < d) ? dof[s] * op[2 * s] : 0.f;
    return dl + xhalf(dl);
}

// the dQ kernels' probability / dS step, query on the lane (lse and delta its scalars): s = dS = p (dp - delta), p = exp(s - lse), 0 for the keys key0 + mfma_row(r, hi) past S
__device__ __forceinline__ void prob_ds_q(f32x16& s, const f32x16& dp, int key0, int S, int hi, float lse, float delta) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float p = key0 + mfma_row(r, hi) < S ? __expf(s[r] - lse) : 0.f;
        s[r] = p * (dp[r] - delta);
    }
}

// ---- host side: what the entry points of both files check, and the launch over the head width
inline bool d_ok(int d) { return d >= 8 && d <= 64 && d % 8 == 0; }
inline bool dw_ok(int d) { return d >= 1 && d <= 64; }      // seld_attnw_*: any width; d % 8 != 0 runs the RAG form at D = 8 ceil(d / 8)
// a row stride covers the H * d columns of all heads; the product in 64 bits: H * d past INT_MAX fits no int stride (and the kernels' H * D stays an int)
inline bool ld_ok(int ld, int H, int d) { return (int64_t)ld >= (int64_t)H * d; }
// workgroups B * H * ceil(S / 64), or -1 where they do not fit a launch; every product in 64 bits and bounded before the next factor
inline int64_t tile_grid(int B, int S, int H) {
    const int64_t bh = (int64_t)B * H, nt = ((int64_t)S + ATTN_TILE - 1) / ATTN_TILE;
    return bh > 0x7fffffff || bh * nt > 0x7fffffff ? -1 : bh * nt;
}

}  // namespace attn_tile

// `launch`(D, ...) with D = the head width d as a constant, d = 8, 16, ..., 64 (d_ok); `launch` is the including file's macro that names the
// kernel's template arguments and its LDS bytes
#define ATTN_DISPATCH_D(d, launch, ...)            \
    switch (d) {                                   \
        case 8: launch(8, __VA_ARGS__); break;     \
        case 16: launch(16, __VA_ARGS__); break;   \
        case 24: launch(24, __VA_ARGS__); break;   \
        case 32: launch(32, __VA_ARGS__); break;   \
        case 40: launch(40, __VA_ARGS__); break;   \
        case 48: launch(48, __VA_ARGS__); break;   \
        case 56: launch(56, __VA_ARGS__); break;   \
        default: launch(64, __VA_ARGS__); break;   \
    }
