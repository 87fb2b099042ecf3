// augment.hip — the batch augmentations of the reference's training pipeline (train.py:157-165), on the device so
// that a batch goes host -> HBM once and is augmented where the step reads it:
//   aug_mask          transforms.mask (transforms.py:6-44): per sample and per `period`-frame segment, zero a random
//                     run of frames (axis -3) and/or of frequency bins (axis -2); the random draws come from the host
//   aug_v2            the sample transforms of trainv2.get_dataset (trainv2.py:120-140) in one pass: random_ups_and_downs' per-sample shift on
//                     the first channels, then the union of up to 16 time masks and 16 frequency masks per `period`-frame segment
//   aug_gather_sign   the channel shuffles with sign flips of foa_intensity_vec_aug / acs_aug (transforms.py:73-114,
//                     159-207): out[b, o, r, i] = sgn[b, r] * in[b, o, src[b, r], i], in place
// Pure data movement: results are bit-identical to the numpy restatement (oracle/transforms_oracle.py).
#include "common.h"

#include <algorithm>
#include <stdint.h>
#include "../../include/seld_hip.h"

namespace {

// x [B, T, F, C]; segment s = t / period of sample b: frames [t_off, t_off + t_size) of the segment and bins
// [f_off, f_off + f_size) (for every frame of the segment) are zeroed.  One thread per (b, t, f): C contiguous floats.
__global__ __launch_bounds__(256) void aug_mask_kernel(float* __restrict__ x, int T, int F, int C, int period, int nseg,
                                                       const int* __restrict__ t_off, const int* __restrict__ t_size,
                                                       const int* __restrict__ f_off, const int* __restrict__ f_size,
                                                       int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int f = (int)(i % F);
    const int64_t bt = i / F;
    const int t = (int)(bt % T), b = (int)(bt / T);
    const int seg = b * nseg + t / period, tt = t % period;
    bool kill = false;
    if (t_off) kill = tt >= t_off[seg] && tt < t_off[seg] + t_size[seg];
    if (f_off) kill = kill || (f >= f_off[seg] && f < f_off[seg] + f_size[seg]);
    if (kill) {
        float* p = x + i * C;
        for (int c = 0; c < C; ++c) p[c] = 0.f;
    }
}

#define AUG_V2_MAX_MASKS 16
#define AUG_V2_MAX_FC 16384            // floats of one frame (F * C): one op byte each in LDS
#define AUG_V2_MAX_FRAMES 1024         // frames of one workgroup's chunk: one flag byte each in LDS
// x [B, T, F, C].  One workgroup per (sample, segment, chunk of `fpc` frames).  It folds its segment's runs into op[e], one byte per float
// of a frame (2: the bin is masked, 1: the channel takes the shift, 0: untouched — the same for every frame), and dead[i], one byte per
// frame of the chunk; then it streams the chunk: a dead frame and a masked float are stored as +0.0f without being read, a word of four
// untouched floats is neither read nor written.  VEC: F * C % 4 == 0 and x is 16-byte aligned, so every frame is.  tpf (a power of two <=
// 256) threads share a frame, 256 / tpf frames are in flight.
template <bool VEC>
__global__ __launch_bounds__(256) void aug_v2_kernel(float* __restrict__ x, int T, int F, int C, int period, int nseg, int nchunk, int fpc, int tpf,
                                                     const float* __restrict__ shift, int n_shift_ch, const int* __restrict__ t_off,
                                                     const int* __restrict__ t_size, int n_t, const int* __restrict__ f_off,
                                                     const int* __restrict__ f_size, int n_f, int nrun) {
    __shared__ __attribute__((aligned(16))) unsigned char op[AUG_V2_MAX_FC];
    __shared__ unsigned char dead[AUG_V2_MAX_FRAMES];
    __shared__ int run[4][AUG_V2_MAX_MASKS];      // t_off, t_end, f_off, f_end
    const int tid = threadIdx.x;
    const int chunk = blockIdx.x % nchunk, seg = blockIdx.x / nchunk;      // seg = b * nseg + s, the tables' column
    const int b = seg / nseg, s = seg - b * nseg;
    if (tid < n_t) { const int o = t_off[(size_t)tid * nrun + seg]; run[0][tid] = o; run[1][tid] = o + t_size[(size_t)tid * nrun + seg]; }
    if (tid >= 64 && tid - 64 < n_f) {
        const int k = tid - 64, o = f_off[(size_t)k * nrun + seg];
        run[2][k] = o; run[3][k] = o + f_size[(size_t)k * nrun + seg];
    }
    __syncthreads();
    const int FC = F * C;
    const bool add = shift != nullptr && n_shift_ch > 0;
    for (int e = tid; e < FC; e += 256) {
        const int bin = e / C, ch = e - bin * C;
        bool kill = false;
        for (int k = 0; k < n_f; ++k) kill = kill || (bin >= run[2][k] && bin < run[3][k]);
        op[e] = kill ? 2 : (add && ch < n_shift_ch ? 1 : 0);
    }
    const int f0 = chunk * fpc, nfr = min(fpc, period - f0);      // frames [f0, f0 + nfr) of the segment
    for (int i = tid; i < nfr; i += 256) {
        bool kill = false;
        for (int k = 0; k < n_t; ++k) kill = kill || (f0 + i >= run[0][k] && f0 + i < run[1][k]);
        dead[i] = kill;
    }
    __syncthreads();
    const float sh = add ? shift[b] : 0.f;
    const int lane = tid & (tpf - 1), fsub = tid / tpf, fpar = 256 / tpf;
    float* base = x + ((size_t)b * T + (size_t)s * period + f0) * FC;
    for (int i = fsub; i < nfr; i += fpar) {
        float* p = base + (size_t)i * FC;
        const bool dd = dead[i];
        if (VEC) {
            for (int j = lane; j < FC / 4; j += tpf) {
                const unsigned w = dd ? 0x02020202u : reinterpret_cast<const unsigned*>(op)[j];
                if (w == 0) continue;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (w != 0x02020202u) v = reinterpret_cast<const float4*>(p)[j];      // a word that is masked whole is not read
                v.x = (w & 0x2u) ? 0.f : ((w & 0x1u) ? v.x + sh : v.x);
                v.y = (w & 0x200u) ? 0.f : ((w & 0x100u) ? v.y + sh : v.y);
                v.z = (w & 0x20000u) ? 0.f : ((w & 0x10000u) ? v.z + sh : v.z);
                v.w = (w & 0x2000000u) ? 0.f : ((w & 0x1000000u) ? v.w + sh : v.w);
                reinterpret_cast<float4*>(p)[j] = v;
            }
        } else {
            for (int j = lane; j < FC; j += tpf) {
                const unsigned w = dd ? 2u : op[j];
                if (w == 0) continue;
                p[j] = (w & 2u) ? 0.f : p[j] + sh;
            }
        }
    }
}

#define AUG_MAX_R 32
// one thread per (b, o, i): reads its R values, writes them back permuted and signed
__global__ __launch_bounds__(256) void aug_gather_sign_kernel(float* __restrict__ x, int64_t outer, int R, int64_t inner,
                                                              const int* __restrict__ src, const float* __restrict__ sgn,
                                                              int64_t n) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= n) return;
    const int64_t i = g % inner, bo = g / inner;
    const int b = (int)(bo / outer);
    float* p = x + bo * R * inner + i;
    float v[AUG_MAX_R];
#pragma unroll
    for (int r = 0; r < AUG_MAX_R; ++r)
        if (r < R) v[r] = p[(int64_t)r * inner];
#pragma unroll
    for (int r = 0; r < AUG_MAX_R; ++r)
        if (r < R) {
            const int s = src[b * R + r];
            float val = 0.f;
#pragma unroll
            for (int q = 0; q < AUG_MAX_R; ++q) val = (q == s) ? v[q] : val;     // register select: no dynamic indexing
            p[(int64_t)r * inner] = sgn[b * R + r] * val;
        }
}

}  // namespace

extern "C" {

int seld_aug_mask(float* x, int B, int T, int F, int C, int period, const int* t_off, const int* t_size, const int* f_off,
                  const int* f_size, void* stream) {
    if (!x || B <= 0 || T <= 0 || F <= 0 || C <= 0 || period <= 0) return SELD_ERR_INVALID;
    if (T % period) return SELD_ERR_INVALID;                 /* transforms.py:39-40: ValueError */
    if ((t_off == nullptr) != (t_size == nullptr) || (f_off == nullptr) != (f_size == nullptr)) return SELD_ERR_INVALID;
    if (!t_off && !f_off) return SELD_OK;
    const int64_t n = (int64_t)B * T * F;
    hipLaunchKernelGGL(aug_mask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, T, F, C, period,
                       T / period, t_off, t_size, f_off, f_size, n);
    return hipGetLastError() == hipSuccess ? SELD_OK : SELD_ERR_HIP;
}

int seld_aug_v2(float* x, int B, int T, int F, int C, int period, const float* shift, int n_shift_ch, const int* t_off, const int* t_size, int n_t,
                const int* f_off, const int* f_size, int n_f, void* stream) {
    if (!x || B <= 0 || T <= 0 || F <= 0 || C <= 0 || period <= 0) return SELD_ERR_INVALID;
    if (T % period) return SELD_ERR_INVALID;                 /* transforms.py:39-40: ValueError */
    if (n_t < 0 || n_t > AUG_V2_MAX_MASKS || n_f < 0 || n_f > AUG_V2_MAX_MASKS || n_shift_ch < 0 || n_shift_ch > C) return SELD_ERR_INVALID;
    if ((n_t > 0 && (!t_off || !t_size)) || (n_f > 0 && (!f_off || !f_size))) return SELD_ERR_INVALID;
    const int64_t nrun = (int64_t)B * (T / period), FC = (int64_t)F * C;
    if (FC > AUG_V2_MAX_FC || nrun > 0x7fffffff / 64) return SELD_ERR_UNSUPPORTED;
    /* the tables are read here, by the host, and by the kernel: a run with a negative size or offset, or one that ends behind its axis,
     * would send the kernel outside the segment */
    for (int64_t i = 0; i < n_t * nrun; ++i)
        if (t_size[i] < 0 || t_off[i] < 0 || (int64_t)t_off[i] + t_size[i] > period) return SELD_ERR_INVALID;
    for (int64_t i = 0; i < n_f * nrun; ++i)
        if (f_size[i] < 0 || f_off[i] < 0 || (int64_t)f_off[i] + f_size[i] > F) return SELD_ERR_INVALID;
    const bool add = shift && n_shift_ch > 0;
    if (!add && n_t == 0 && n_f == 0) return SELD_OK;
    /* ~16 KiB of x per workgroup, fewer and larger chunks once that gives more than 2048 workgroups; a chunk's frame flags fit the LDS */
    int64_t nchunk = std::max<int64_t>(1, std::min<int64_t>(period, ((int64_t)period * FC * 4 + 16383) / 16384));
    if (nrun * nchunk > 2048) nchunk = std::max<int64_t>(1, 2048 / nrun);
    int fpc = (int)((period + nchunk - 1) / nchunk);
    if (fpc > AUG_V2_MAX_FRAMES) fpc = AUG_V2_MAX_FRAMES;
    nchunk = (period + fpc - 1) / fpc;
    const bool vec = FC % 4 == 0 && ((uintptr_t)x & 15) == 0;
    const int64_t per = vec ? FC / 4 : FC;
    int tpf = 1;
    while (tpf < per && tpf < 256) tpf <<= 1;
    const dim3 grid((unsigned)(nrun * nchunk));
    if (vec)
        hipLaunchKernelGGL((aug_v2_kernel<true>), grid, dim3(256), 0, (hipStream_t)stream, x, T, F, C, period, T / period, (int)nchunk, fpc, tpf, shift,
                           n_shift_ch, t_off, t_size, n_t, f_off, f_size, n_f, (int)nrun);
    else
        hipLaunchKernelGGL((aug_v2_kernel<false>), grid, dim3(256), 0, (hipStream_t)stream, x, T, F, C, period, T / period, (int)nchunk, fpc, tpf, shift,
                           n_shift_ch, t_off, t_size, n_t, f_off, f_size, n_f, (int)nrun);
    return hipGetLastError() == hipSuccess ? SELD_OK : SELD_ERR_HIP;
}

int seld_aug_gather_sign(float* x, int B, int64_t outer, int R, int64_t inner, const int* src, const float* sgn, void* stream) {
    if (!x || !src || !sgn || B <= 0 || outer <= 0 || inner <= 0 || R <= 0) return SELD_ERR_INVALID;
    if (R > AUG_MAX_R) return SELD_ERR_UNSUPPORTED;
    const int64_t n = (int64_t)B * outer * inner;
    hipLaunchKernelGGL(aug_gather_sign_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, outer, R,
                       inner, src, sgn, n);
    return hipGetLastError() == hipSuccess ? SELD_OK : SELD_ERR_HIP;
}

}  // extern "C"
