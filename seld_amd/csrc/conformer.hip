// conformer.hip — what the reference's conformer_encoder_block (modules.py:410-508) needs beyond attention.hip and module_ops.hip: the
// convolution module's GLU + depthwise Conv1D(groups = emb, kernel_size k, 'same') (modules.py:476-486), forward and backward, and two small
// movers (the positional table's broadcast add, modules.py:450; the head-major weights of layers.MultiHeadAttention_, layers.py:148-175, to
// and from the [D, H dk] form a GEMM takes).  C ABI "seld_dwconv1d_*" / "seld_pos_add" / "seld_head_permute": asynchronous on the caller's
// stream, no allocation, caller scratch.  The glu = 0 form is attention_block's depthwise convolution (modules.py:603-611).
//
// A depthwise convolution has no reuse across channels, so the channel is the lane: a workgroup of 512 threads = 64 channels x 8 time groups
// owns a tile of DW_TT = 128 frames of one clip.  The tile plus its k - 1 halo frames is staged ONCE into LDS, [frame][64 channels] (a wave
// reads 64 consecutive floats of a row: coalesced from memory, conflict-free in LDS); with glu = 1 the loader forms a * sigmoid(b) from the
// two halves of the row, so the gated tensor never exists in memory.  The taps w[t][c] sit in LDS beside it.  A thread then produces 16
// consecutive frames of its channel from a 16-float register window that slides one frame per tap: one LDS read of the tile and one of the
// tap per 16 multiply-adds.  The input gradient is the same kernel on dy with the taps reversed and the padding split mirrored; its epilogue
// applies the GLU's derivative from u (re-read, cache-hot) and writes both halves of du.
//
// dw[t][c] = sum_{b,s} dy[b,s,c] g[b,s-pl+t,c] and dbias[c] = sum dy are reduced in two stages: a workgroup (64 channels, one of at most
// DW_SLOTS slots) walks the 64-frame tiles slot, slot + slots, ..., staging dy and the gated halo tile, and a thread keeps 8 taps of its channel
// in registers with the same sliding window (the tile's frames are split over the thread groups the taps leave free, and folded through LDS in
// a fixed order); the slot's (k + 1) x C partials go to scratch and a second kernel adds the slots in order, in double.  No atomics: two runs
// give the same bits.  Every row offset is formed in 64 bits.
#include "common.h"
#include "../../include/seld_hip.h"
#include <math.h>

namespace {

#define DW_CH 64          // channels per workgroup = lanes of a wave
#define DW_TT 128         // frames per workgroup of the forward / input-gradient kernel (16 per thread)
#define DW_WT 64          // frames per tile of the weight-gradient kernel
#define DW_SLOTS 512      // first-stage partial sums of dw / dbias
#define DW_KMAX 64

// sigmoid(b) and its derivative without cancellation or overflow at any b: e = exp(-|b|) <= 1
__device__ __forceinline__ void sigmoid_and_slope(float b, float& sg, float& ds) {
    const float e = expf(-fabsf(b)), r = 1.f / (1.f + e);
    sg = b >= 0.f ? r : e * r;
    ds = e * r * r;
}

template <bool GLU>
__device__ __forceinline__ float load_gated(const float* __restrict__ u, int ld, size_t row, int c, int C) {
    const float* p = u + row * (size_t)ld + c;
    float a = p[0];
    if (GLU) {
        float sg, ds;
        sigmoid_and_slope(p[C], sg, ds);
        a *= sg;
    }
    return a;
}

// BWD 0: out[b,s,c] = bias[c] + sum_t w[t,c] g[b, s - front + t, c], g = GLU ? src[..c] sigmoid(src[..C + c]) : src[..c]
// BWD 1: dg[b,s,c] = sum_t w[k-1-t,c] src[b, s - front + t, c] (src = dy, front = k - 1 - pl); out = du: GLU ? both halves from u : dg
template <bool GLU, bool BWD>
__global__ __launch_bounds__(512) void dwconv_tile_kernel(const float* __restrict__ src, int lds, const float* __restrict__ w,
                                                          const float* __restrict__ bias, const float* __restrict__ u, int ldu,
                                                          float* __restrict__ out, int ldo, int S, int C, int k, int front, int ntt, int nct) {
    extern __shared__ float sm[];
    const int KP = (k + 7) & ~7, rows = DW_TT + KP;      // taps padded to a multiple of 8 with zeros; one row more than the window ever uses
    float* gt = sm;                    // [rows][64]
    float* wt = sm + rows * DW_CH;     // [KP][64]
    const int cl = threadIdx.x & 63, grp = threadIdx.x >> 6;
    int bid = blockIdx.x;
    const int ct = bid % nct;
    bid /= nct;
    const int tt = bid % ntt, b = bid / ntt;
    const int c = ct * DW_CH + cl;
    const bool cok = c < C;
    const int s0 = tt * DW_TT;
    const size_t row0 = (size_t)b * S;
    for (int r = grp; r < rows; r += 8) {
        const int s = s0 - front + r;
        float v = 0.f;
        if (cok && s >= 0 && s < S && r < DW_TT + k - 1) v = load_gated<GLU && !BWD>(src, lds, row0 + s, c, C);
        gt[r * DW_CH + cl] = v;
    }
    for (int t = grp; t < KP; t += 8) wt[t * DW_CH + cl] = cok && t < k ? w[(size_t)(BWD ? k - 1 - t : t) * C + c] : 0.f;
    __syncthreads();
    float acc[16], win[16];
    const float* gp = gt + grp * 16 * DW_CH + cl;
#pragma unroll
    for (int j = 0; j < 16; ++j) { acc[j] = 0.f; win[j] = gp[j * DW_CH]; }
    for (int t0 = 0; t0 < KP; t0 += 8) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int t = t0 + i;
            const float wv = wt[t * DW_CH + cl];
#pragma unroll
            for (int j = 0; j < 16; ++j) acc[j] = fmaf(wv, win[j], acc[j]);
#pragma unroll
            for (int j = 0; j < 15; ++j) win[j] = win[j + 1];
            win[15] = gp[(t + 16) * DW_CH];      // frame 16 grp + t + 16 of the tile: at most row DW_TT + KP - 1
        }
    }
    if (!cok) return;
    const float bv = BWD ? 0.f : bias[c];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int s = s0 + grp * 16 + j;
        if (s >= S) break;
        float* o = out + (row0 + s) * (size_t)ldo + c;
        if (BWD && GLU) {
            const float* up = u + (row0 + s) * (size_t)ldu + c;
            float sg, ds;
            sigmoid_and_slope(up[C], sg, ds);
            o[0] = acc[j] * sg;
            o[C] = acc[j] * up[0] * ds;
        } else {
            o[0] = acc[j] + bv;
        }
    }
}

// first stage of dw / dbias: part[slot][t][c] (t < k) and part[slot][k][c] (dbias) over the tiles slot, slot + nslots, ...
template <bool GLU>
__global__ __launch_bounds__(512) void dwconv_wgrad_kernel(const float* __restrict__ u, int ldu, const float* __restrict__ dy,
                                                           float* __restrict__ part, int S, int C, int k, int pl, int ntt, int64_t ntiles) {
    extern __shared__ float sm[];
    const int KP = (k + 7) & ~7, rows = DW_WT + KP;
    const int nchunk = KP >> 3, nsplit = 8 / nchunk, L = DW_WT / nsplit;      // 8 taps per thread; the free thread groups split the tile's frames
    float* gt = sm;                    // [rows][64] the gated input, frames s0 - pl ..
    float* dt = sm + rows * DW_CH;     // [64][64] dy, frames s0 ..
    const int cl = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const int c = blockIdx.x * DW_CH + cl;
    const bool cok = c < C, active = grp < nchunk * nsplit;
    const int t0 = (grp / nsplit) * 8, sA = (grp % nsplit) * L;
    float acc[8], bsum = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    for (int64_t tile = blockIdx.y; tile < ntiles; tile += gridDim.y) {
        const int s0 = (int)(tile % ntt) * DW_WT;
        const size_t row0 = (size_t)(tile / ntt) * S;
        __syncthreads();
        for (int r = grp; r < rows; r += 8) {
            const int s = s0 - pl + r;
            float v = 0.f;
            if (cok && s >= 0 && s < S && r < DW_WT + k - 1) v = load_gated<GLU>(u, ldu, row0 + s, c, C);
            gt[r * DW_CH + cl] = v;
        }
        for (int r = grp; r < DW_WT; r += 8) {
            const int s = s0 + r;
            const float v = cok && s < S ? dy[(row0 + s) * (size_t)C + c] : 0.f;
            dt[r * DW_CH + cl] = v;
            bsum += v;
        }
        __syncthreads();
        if (active) {
            // dw[t0 + j] += dy[s] g[s - pl + t0 + j]: row s + t0 + j of the tile; the window slides with s
            const float* gp = gt + (sA + t0) * DW_CH + cl;
            const float* dp = dt + sA * DW_CH + cl;
            float win[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) win[j] = gp[j * DW_CH];
            for (int ss = 0; ss < L; ss += 8) {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const float d = dp[(ss + i) * DW_CH];
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[j] = fmaf(d, win[j], acc[j]);
#pragma unroll
                    for (int j = 0; j < 7; ++j) win[j] = win[j + 1];
                    win[7] = gp[(ss + i + 8) * DW_CH];      // at most row 63 + 8 + KP - 8 < rows
                }
            }
        }
    }
    __syncthreads();
    float* red = sm;                        // [8 groups][8 taps][64]
    float* redb = sm + 8 * 8 * DW_CH;       // [8 groups][64]     (4608 floats <= rows * 64)
#pragma unroll
    for (int j = 0; j < 8; ++j) red[(grp * 8 + j) * DW_CH + cl] = active ? acc[j] : 0.f;
    redb[grp * DW_CH + cl] = bsum;
    __syncthreads();
    if (!cok) return;
    float* P = part + (size_t)blockIdx.y * (size_t)(k + 1) * C;
    for (int t = grp; t < k; t += 8) {
        const int g0 = (t >> 3) * nsplit, j = t & 7;
        float s = 0.f;
        for (int sp = 0; sp < nsplit; ++sp) s += red[((g0 + sp) * 8 + j) * DW_CH + cl];
        P[(size_t)t * C + c] = s;
    }
    if (grp == 0) {
        float s = 0.f;
        for (int g = 0; g < 8; ++g) s += redb[g * DW_CH + cl];
        P[(size_t)k * C + c] = s;
    }
}

// second stage: element e of [k + 1][C] summed over the slots in slot order
__global__ __launch_bounds__(256) void dwconv_fold_kernel(const float* __restrict__ part, int nslots, int64_t n, int64_t nw, float* __restrict__ dw,
                                                          float* __restrict__ dbias) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    double a = 0.0;
    for (int sidx = 0; sidx < nslots; ++sidx) a += part[(size_t)sidx * n + e];
    if (e < nw) dw[e] = (float)a;
    else dbias[e - nw] = (float)a;
}

// x[b, s, :] += enc[s, :]
__global__ __launch_bounds__(256) void pos_add_kernel(float* __restrict__ x, const float* __restrict__ enc, int64_t n, int64_t sd) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < n) x[e] += enc[e % sd];
}

// mode 0: dst[d][h][o] = src[h][d][o]; mode 1: dst[h][d][o] = src[d][h][o]
__global__ __launch_bounds__(256) void head_permute_kernel(const float* __restrict__ src, float* __restrict__ dst, int H, int D, int dk, int mode,
                                                           int64_t n) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const int o = (int)(e % dk);
    const int64_t q = e / dk;
    int64_t from;
    if (mode == 0) { const int h = (int)(q % H); const int64_t d = q / H; from = ((int64_t)h * D + d) * dk + o; }
    else { const int64_t d = q % D, h = q / D; from = (d * H + h) * dk + o; }
    dst[e] = src[from];
}

inline bool dw_sizes_ok(int B, int S, int C, int k) { return B >= 1 && S >= 1 && C >= 1 && k >= 1 && k <= DW_KMAX; }
// workgroups of the tile kernel, or -1 where they do not fit a launch; every product in 64 bits and bounded before the next factor
inline int64_t dw_grid(int B, int S, int C) {
    const int64_t nct = ((int64_t)C + DW_CH - 1) / DW_CH, ntt = ((int64_t)S + DW_TT - 1) / DW_TT;
    if (S > 0x7fffff00 || nct * ntt > 0x7fffffff || nct * ntt * B > 0x7fffffff) return -1;      // (a tile's frame index s0 + row stays an int)
    return nct * ntt * B;
}
inline int64_t dw_tiles(int B, int S) { return (int64_t)B * (((int64_t)S + DW_WT - 1) / DW_WT); }
inline int dw_slots(int B, int S) { const int64_t t = dw_tiles(B, S); return (int)(t < DW_SLOTS ? t : DW_SLOTS); }
inline size_t tile_lds(int k) { const int KP = (k + 7) & ~7; return (size_t)(DW_TT + 2 * KP) * DW_CH * sizeof(float); }
inline size_t wgrad_lds(int k) { const int KP = (k + 7) & ~7; return (size_t)(2 * DW_WT + KP) * DW_CH * sizeof(float); }

}  // namespace

extern "C" {

int seld_dwconv1d_fwd(const float* u, int ldu, const float* w, const float* bias, float* y, int B, int S, int C, int k, int glu, void* stream) {
    if (!u || !w || !bias || !y || !dw_sizes_ok(B, S, C, k) || (glu != 0 && glu != 1) || (int64_t)ldu < (int64_t)(glu + 1) * C)
        return SELD_ERR_INVALID;
    const int64_t grid = dw_grid(B, S, C);
    if (grid < 0) return SELD_ERR_UNSUPPORTED;
    const int nct = (C + DW_CH - 1) / DW_CH, ntt = (int)(((int64_t)S + DW_TT - 1) / DW_TT), pl = (k - 1) / 2;
    if (glu)
        hipLaunchKernelGGL((dwconv_tile_kernel<true, false>), dim3((unsigned)grid), dim3(512), tile_lds(k), (hipStream_t)stream, u, ldu, w, bias,
                           (const float*)nullptr, 0, y, C, S, C, k, pl, ntt, nct);
    else
        hipLaunchKernelGGL((dwconv_tile_kernel<false, false>), dim3((unsigned)grid), dim3(512), tile_lds(k), (hipStream_t)stream, u, ldu, w, bias,
                           (const float*)nullptr, 0, y, C, S, C, k, pl, ntt, nct);
    return ok();
}

/* floats of caller scratch seld_dwconv1d_bwd takes: the first-stage partial sums of dw / dbias, [slots <= 512][k + 1][C] */
int64_t seld_dwconv1d_bwd_scratch(int B, int S, int C, int k) {
    if (!dw_sizes_ok(B, S, C, k) || dw_grid(B, S, C) < 0) return -1;
    return (int64_t)dw_slots(B, S) * (k + 1) * C;
}

int seld_dwconv1d_bwd(const float* u, int ldu, const float* w, const float* dy, float* du, int lddu, float* dw, float* dbias, float* scratch, int B,
                      int S, int C, int k, int glu, void* stream) {
    if (!u || !w || !dy || !du || !dw || !dbias || !scratch || !dw_sizes_ok(B, S, C, k) || (glu != 0 && glu != 1) ||
        (int64_t)ldu < (int64_t)(glu + 1) * C || (int64_t)lddu < (int64_t)(glu + 1) * C)
        return SELD_ERR_INVALID;
    const int64_t grid = dw_grid(B, S, C);
    if (grid < 0) return SELD_ERR_UNSUPPORTED;
    const int nct = (C + DW_CH - 1) / DW_CH, ntt = (int)(((int64_t)S + DW_TT - 1) / DW_TT), pl = (k - 1) / 2;
    const int nwt = (int)(((int64_t)S + DW_WT - 1) / DW_WT), nslots = dw_slots(B, S);
    const int64_t nw = (int64_t)k * C, n = nw + C;
    hipStream_t st = (hipStream_t)stream;
    if (glu) {
        hipLaunchKernelGGL((dwconv_tile_kernel<true, true>), dim3((unsigned)grid), dim3(512), tile_lds(k), st, dy, C, w, (const float*)nullptr, u, ldu, du,
                           lddu, S, C, k, k - 1 - pl, ntt, nct);
        hipLaunchKernelGGL((dwconv_wgrad_kernel<true>), dim3(nct, nslots), dim3(512), wgrad_lds(k), st, u, ldu, dy, scratch, S, C, k, pl, nwt,
                           dw_tiles(B, S));
    } else {
        hipLaunchKernelGGL((dwconv_tile_kernel<false, true>), dim3((unsigned)grid), dim3(512), tile_lds(k), st, dy, C, w, (const float*)nullptr, u, ldu,
                           du, lddu, S, C, k, k - 1 - pl, ntt, nct);
        hipLaunchKernelGGL((dwconv_wgrad_kernel<false>), dim3(nct, nslots), dim3(512), wgrad_lds(k), st, u, ldu, dy, scratch, S, C, k, pl, nwt,
                           dw_tiles(B, S));
    }
    hipLaunchKernelGGL(dwconv_fold_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, scratch, nslots, n, nw, dw, dbias);
    return ok();
}

int seld_pos_add(float* x, const float* enc, int B, int S, int D, void* stream) {
    if (!x || !enc || B < 1 || S < 1 || D < 1) return SELD_ERR_INVALID;
    const int64_t sd = (int64_t)S * D, n = sd * B;      // sd is bounded before the next factor
    if (sd > 0x7fffffff || (n + 255) / 256 > 0x7fffffff) return SELD_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(pos_add_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, enc, n, sd);
    return ok();
}

int seld_head_permute(const float* src, float* dst, int H, int D, int dk, int mode, void* stream) {
    if (!src || !dst || H < 1 || D < 1 || dk < 1 || (mode != 0 && mode != 1)) return SELD_ERR_INVALID;
    const int64_t hd = (int64_t)H * D, n = hd * dk;
    if (hd > 0x7fffffff || (n + 255) / 256 > 0x7fffffff) return SELD_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(head_permute_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src, dst, H, D, dk, mode, n);
    return ok();
}

}  // extern "C"
