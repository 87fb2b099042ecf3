// tdm.hip — time-domain mixing, the training-set regeneration of the reference's train.get_tdm_dataset (data_loader.TDM_aug,
// data_loader.py:188-234), on the device: single-class "noise" clips of a bank are added into the training clips, label frame by label
// frame, where the labels leave room.  The host draws a plan int32 [B][K][4] = (cls, st, offset, td_offset) per clip: insertion k adds `st`
// label frames of class `cls`, taken from frame `td_offset` of that class's bank track, at frame `offset` of the clip.
//   aug_tdm_labels   the label bookkeeping: one workgroup per clip walks its K insertions IN ORDER (an insertion's validity depends on what the
//                    earlier ones added): v[f] = (sum_c activity[off+f][c] < max_per_frame) * (1 - activity[off+f][cls]), stored to `valid`,
//                    then y[off+f][:] += bank_y[cls][td+f][:] * v[f]
//   aug_tdm_mix      the waveforms: one workgroup per (clip, label frame) adds, in plan order, bank_x[cls][:, (td+f-off)*spf ...] * v[f-off] of
//                    every insertion that covers its frame; a sample is read once and written once
// Multiply, then add, never contracted to an FMA: the bits of the reference's `y[i] += pad(tdm_y * v)`, `x[i] += pad(tdm_x * v)` applied one
// insertion after the other (tests/tdm_oracle.py).  No atomics, fixed order: two calls give the same bits.
#include "common.h"

#include <stdint.h>
#include "../../include/seld_hip.h"

#pragma clang fp contract(off)

#define TDM_MAX_K 32                 // insertions per clip (the reference draws at most 5)
#define TDM_MAX_BLOCKS 0xFFFFFF      // workgroups of 256 threads one launch takes (grid * block stays below 2^32)

namespace {

// One plan row, checked against everything a kernel is about to index with it.  `rows` = label frames of the class's bank track (labels kernel)
// or the frames its packed waveform holds (mix kernel).
struct TdmRow { int cls, st, off, td; };
__device__ __forceinline__ TdmRow tdm_row(const int* __restrict__ plan, int64_t i) {
    const int4 r = *reinterpret_cast<const int4*>(plan + 4 * i);      // plan rows are 16 bytes, the base is checked by the entry points
    return TdmRow{r.x, r.y, r.z, r.w};
}
__device__ __forceinline__ bool tdm_row_in_clip(const TdmRow& r, int T, int n_cls, int ld_valid) {
    return r.cls >= 0 && r.cls < n_cls && r.st >= 1 && r.st <= T && r.st <= ld_valid && r.off >= 0 && r.off <= T - r.st && r.td >= 0;
}

// y [B][T][W], W = 4 nc: [activity | x | y | z].  One workgroup per clip.
__global__ __launch_bounds__(256) void aug_tdm_labels_kernel(float* __restrict__ y, int T, int W, const float* __restrict__ bank_y,
                                                             const int64_t* __restrict__ bank_row0, const int64_t* __restrict__ bank_rows, int n_cls,
                                                             const int* __restrict__ plan, int K, float max_per_frame, float* __restrict__ valid,
                                                             int ld_valid) {
    const int b = blockIdx.x, tid = threadIdx.x, nc = W / 4;
    float* yb = y + (int64_t)b * T * W;
    for (int k = 0; k < K; ++k) {
        const TdmRow r = tdm_row(plan, (int64_t)b * K + k);      // the same for every thread: the branches below are workgroup-uniform
        float* v = valid + ((int64_t)b * K + k) * ld_valid;
        bool good = tdm_row_in_clip(r, T, n_cls, ld_valid);
        int64_t row0 = 0;
        if (good) {
            const int64_t rows = bank_rows[r.cls];
            row0 = bank_row0[r.cls];
            good = row0 >= 0 && (int64_t)r.td + r.st <= rows;
        }
        const int st = good ? r.st : 0;
        for (int f = tid; f < ld_valid; f += 256) {
            float vf = 0.f;
            if (f < st) {
                const float* row = yb + (int64_t)(r.off + f) * W;
                float s = 0.f;
                for (int c = 0; c < nc; ++c) s = s + row[c];
                vf = (s < max_per_frame ? 1.f : 0.f) * (1.f - row[r.cls]);
            }
            v[f] = vf;
        }
        __syncthreads();      // every v[f] is formed from the labels as the earlier insertions left them, and is visible to the workgroup
        if (st > 0) {
            const float* src = bank_y + (row0 + r.td) * W;
            float* dst = yb + (int64_t)r.off * W;
            const int64_t n = (int64_t)st * W;
            for (int64_t e = tid; e < n; e += 256) {
                const float p = src[e] * v[e / W];
                dst[e] = dst[e] + p;
            }
        }
        __syncthreads();      // the next insertion reads these rows
    }
}

// x [B][C][N], one workgroup per (clip b, label frame f): samples [f spf, (f+1) spf) of the C channels.  bank_x: class k's waveform is the block
// [C][n_k] that starts at float bank_s0[k]; bank_s0 has n_cls + 1 entries, so n_k = (bank_s0[k+1] - bank_s0[k]) / C.  VEC: spf, N, and the three
// base pointers allow float4 accesses of x; a class whose block does not (bank_s0[k] or n_k not a multiple of 4) is read with scalar loads.
template <bool VEC>
__global__ __launch_bounds__(256) void aug_tdm_mix_kernel(const float* x_in, float* x_out /* may be x_in */, int C, int64_t N, int T, int spf,
                                                          const float* __restrict__ bank_x, const int64_t* __restrict__ bank_s0, int n_cls,
                                                          const int* __restrict__ plan, int K, const float* __restrict__ valid, int ld_valid) {
    __shared__ int64_t s_src[TDM_MAX_K];       // float offset in bank_x of the class's channel 0 at this frame
    __shared__ int64_t s_stride[TDM_MAX_K];    // n_k: floats between two channels
    __shared__ float s_v[TDM_MAX_K];
    __shared__ int s_cov[TDM_MAX_K];           // 1: covers this frame; 2: covers it and the source takes float4 loads
    const int tid = threadIdx.x;
    const int b = blockIdx.x / T, f = blockIdx.x - b * T;
    if (tid < K) {
        const TdmRow r = tdm_row(plan, (int64_t)b * K + tid);
        int cov = 0;
        if (tdm_row_in_clip(r, T, n_cls, ld_valid) && f >= r.off && f < r.off + r.st) {
            const int64_t s0 = bank_s0[r.cls], nk = (bank_s0[r.cls + 1] - s0) / C;
            if (s0 >= 0 && ((int64_t)r.td + r.st) * spf <= nk) {
                const int64_t src = s0 + ((int64_t)r.td + (f - r.off)) * spf;
                s_src[tid] = src;
                s_stride[tid] = nk;
                s_v[tid] = valid[((int64_t)b * K + tid) * ld_valid + (f - r.off)];
                cov = ((src | nk) & 3) == 0 ? 2 : 1;
            }
        }
        s_cov[tid] = cov;
    }
    __syncthreads();
    int any = 0;
    for (int k = 0; k < K; ++k) any |= s_cov[k];
    const bool in_place = x_out == x_in;
    if (!any && in_place) return;
    const int64_t clip = (int64_t)b * C * N, at = (int64_t)f * spf;
    if (VEC) {
        const int q = spf / 4, n = C * q;
        for (int e = tid; e < n; e += 256) {
            const int c = e / q, j = e - c * q;
            const int64_t i = clip + (int64_t)c * N + at + 4 * j;
            float4 a = *reinterpret_cast<const float4*>(x_in + i);
            for (int k = 0; k < K; ++k) {
                const int cov = s_cov[k];
                if (!cov) continue;
                const float* t = bank_x + s_src[k] + (int64_t)c * s_stride[k] + 4 * j;
                float4 w;
                if (cov == 2) w = *reinterpret_cast<const float4*>(t);
                else w = make_float4(t[0], t[1], t[2], t[3]);
                const float v = s_v[k];
                const float p0 = w.x * v, p1 = w.y * v, p2 = w.z * v, p3 = w.w * v;
                a.x = a.x + p0; a.y = a.y + p1; a.z = a.z + p2; a.w = a.w + p3;
            }
            *reinterpret_cast<float4*>(x_out + i) = a;
        }
    } else {
        const int n = C * spf;
        for (int e = tid; e < n; e += 256) {
            const int c = e / spf, j = e - c * spf;
            const int64_t i = clip + (int64_t)c * N + at + j;
            float a = x_in[i];
            for (int k = 0; k < K; ++k) {
                if (!s_cov[k]) continue;
                const float p = bank_x[s_src[k] + (int64_t)c * s_stride[k] + j] * s_v[k];
                a = a + p;
            }
            x_out[i] = a;
        }
    }
    if (!in_place && f == T - 1) {      // the samples behind the last label frame are copied as they are
        const int64_t tail = N - (int64_t)T * spf;
        for (int c = 0; c < C; ++c)
            for (int64_t j = tid; j < tail; j += 256) {
                const int64_t i = clip + (int64_t)c * N + (int64_t)T * spf + j;
                x_out[i] = x_in[i];
            }
    }
}

}  // namespace

extern "C" {

int seld_aug_tdm_labels(float* y, int B, int T, int W, const float* bank_y, const int64_t* bank_row0, const int64_t* bank_rows, int n_cls,
                        const int32_t* plan, int K, int max_per_frame, float* valid, int ld_valid, void* stream) {
    if (!y || !bank_y || !bank_row0 || !bank_rows) return SELD_ERR_INVALID;
    if (B < 1 || T < 1 || W < 1 || n_cls < 1 || W % 4 != 0 || K < 0 || ld_valid < 1) return SELD_ERR_INVALID;
    if (n_cls > W / 4) return SELD_ERR_INVALID;      // a bank class is a label class: the kernel reads activity column `cls`
    if (K > TDM_MAX_K || B > TDM_MAX_BLOCKS) return SELD_ERR_UNSUPPORTED;
    if (K == 0) return SELD_OK;
    if (!plan || !valid || ((uintptr_t)plan & 15)) return SELD_ERR_INVALID;
    hipLaunchKernelGGL(aug_tdm_labels_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, y, T, W, bank_y, bank_row0, bank_rows, n_cls,
                       plan, K, (float)max_per_frame, valid, ld_valid);
    return ok();
}

int seld_aug_tdm_mix(const float* x_in, float* x_out, int B, int C, int64_t N, int T, int spf, const float* bank_x, const int64_t* bank_s0, int n_cls,
                     const int32_t* plan, int K, const float* valid, int ld_valid, void* stream) {
    if (!x_in || !x_out || !bank_x || !bank_s0) return SELD_ERR_INVALID;
    if (B < 1 || C < 1 || T < 1 || spf < 1 || n_cls < 1 || K < 0 || ld_valid < 1) return SELD_ERR_INVALID;
    if (N < (int64_t)T * spf) return SELD_ERR_INVALID;
    if (K > TDM_MAX_K || (int64_t)B * T > TDM_MAX_BLOCKS || (int64_t)C * spf > 0x7fffffff) return SELD_ERR_UNSUPPORTED;
    if (K == 0 && x_out == x_in) return SELD_OK;
    if (K > 0 && (!plan || !valid || ((uintptr_t)plan & 15))) return SELD_ERR_INVALID;
    const bool vec = spf % 4 == 0 && N % 4 == 0 && (((uintptr_t)x_in | (uintptr_t)x_out | (uintptr_t)bank_x) & 15) == 0;
    const dim3 grid((unsigned)((int64_t)B * T));
    if (vec)
        hipLaunchKernelGGL((aug_tdm_mix_kernel<true>), grid, dim3(256), 0, (hipStream_t)stream, x_in, x_out, C, N, T, spf, bank_x, bank_s0, n_cls, plan, K,
                           valid, ld_valid);
    else
        hipLaunchKernelGGL((aug_tdm_mix_kernel<false>), grid, dim3(256), 0, (hipStream_t)stream, x_in, x_out, C, N, T, spf, bank_x, bank_s0, n_cls, plan, K,
                           valid, ld_valid);
    return ok();
}

}  // extern "C"
