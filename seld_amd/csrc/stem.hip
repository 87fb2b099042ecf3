// stem.hip — the front of models.conv_temporal (reference models.py:54-66): Conv2D(filters, k, 'same') on the few input channels of the
// feature tensor, and MaxPooling2D(pool, strides = pool, 'same' | 'valid').  C ABI "seld_stem_*" / "seld_pool2d_*" under the seld_m_*
// contract (module_ops.hip): NHWC fp32, asynchronous on the caller's stream, no allocation, caller-provided scratch.
//
// seld_stem_conv_fwd — no im2col buffer.  A workgroup owns 16 image rows x 32 columns x 32 filters; the halo patch (16 + k - 1) x (32 + k - 1)
//   pixels is staged ONCE in LDS as three bf16 planes of CP channel slots per pixel (CP = 8 for Cin <= 7, 16 otherwise; the slots past Cin and
//   the pixels outside the image are zeros, so the product loop has no edge branches).  The reduction index is tap * CP + slot: the 8
//   consecutive k of a bf16 A fragment are one pixel's channel vector, a 16-byte LDS read at (row + dy, column + dx).  Wave w owns tile rows
//   4 w .. 4 w + 3: four 32 x 32 accumulators that share the three B fragments of a k-step, which a lane builds in registers from 8 kernel
//   values (read through the cache: the kernel is at most 7 * 7 * 16 * F floats and every workgroup walks it in the same order).  Six
//   products per fp32 product, fp32 accumulation (sb_tile.h); the bias is added in the epilogue.
// seld_stem_conv_wgrad — the reduction runs over the pixels, so the operands are used as they lie: exact fp32 MFMA (32 x 32 x 2), A[i][p] =
//   the patch value of kernel row i = tap * Cin + c at pixel p (one 4-byte LDS read at a per-lane offset), B[p][f] = dz.  Row k k Cin meets a
//   constant 1.0 and yields the bias gradient.  Stage one: at most 512 workgroups walk the 8 x 32 tiles (patch and dz staged in LDS) in a fixed order and write one partial
//   [k k Cin + 1][F] each; stage two adds the partials in ascending order.  No atomics: two runs give the same bits.
// seld_pool2d_fwd / _bwd — one thread per output (forward) or input (backward) element, four channels at a time where C % 4 == 0.
#include "common.h"
#include "sb_tile.h"

namespace {

constexpr int FWD_TH = 16, FWD_TW = 32;      // forward tile: image rows x columns (x 32 filters)
constexpr int WG_TH = 8, WG_TW = 32;         // weight-gradient tile
constexpr int WG_MAXJ = 7;                   // 32-row chunks of the kernel matrix per wave: 4 * 7 * 32 >= 7 * 7 * 16 + 1
constexpr int WG_MAX_GROUPS = 512;           // first-stage workgroups (= partials) per filter group: two per CU, one staging while the other multiplies
constexpr int STEM_TAB = 128;                // k-step table entries: 2 * ceil(49 * 16 / 16) = 98

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool al4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

// ------------------------------------------------------------------------------------------------ Conv2D forward
template <int CP>
__global__ __launch_bounds__(256) void stem_conv_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                            float* __restrict__ z, int H, int W, int Cin, int k, int F, int tilesH, int tilesW) {
    extern __shared__ __attribute__((aligned(16))) unsigned char stem_smem[];
    int* tab = reinterpret_cast<int*>(stem_smem);                                      // [NS][2]: patch offset of (k-step, half), -1: past the last tap
    unsigned short* patch = reinterpret_cast<unsigned short*>(stem_smem + STEM_TAB * sizeof(int));   // [3][PH][PW][CP]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kg = lane >> 5, li = lane & 31;
    const int pad = k >> 1, KK = k * k;
    const int PH = FWD_TH + k - 1, PW = FWD_TW + k - 1;
    const int PLANE = PH * PW * CP;
    const int NS = (KK * CP + 15) / 16;
    int t = blockIdx.x;
    const int tw = t % tilesW; t /= tilesW;
    const int th = t % tilesH;
    const int b = t / tilesH;
    const int h0 = th * FWD_TH, w0 = tw * FWD_TW;
    const int f = blockIdx.y * 32 + li;
    const bool fok = f < F;
    if (tid < 2 * NS) {
        const int kk = 8 * tid, tap = kk / CP;
        tab[tid] = tap < KK ? ((tap / k) * PW + tap % k) * CP + kk % CP : -1;
    }
    // ---- the halo patch: every pixel of it is written (zeros outside the image and in the slots past Cin)
    for (int idx = tid; idx < PH * PW; idx += 256) {
        const int pr = idx / PW, pc = idx - pr * PW;
        const int h = h0 - pad + pr, wv = w0 - pad + pc;
        const bool ok = h >= 0 && h < H && wv >= 0 && wv < W;
        const float* p = x + (ok ? ((size_t)((size_t)b * H + h) * W + wv) * Cin : 0);
        float v[CP];
#pragma unroll
        for (int c = 0; c < CP; ++c) v[c] = (ok && c < Cin) ? p[c < Cin ? c : 0] : 0.f;
        unsigned short* d = patch + (size_t)idx * CP;
#pragma unroll
        for (int q = 0; q < CP / 8; ++q) {
            unsigned h_[4], m_[4], l_[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) split3_pair(v[8 * q + 2 * i], v[8 * q + 2 * i + 1], h_[i], m_[i], l_[i]);
            const u32x4 hv = {h_[0], h_[1], h_[2], h_[3]}, mv = {m_[0], m_[1], m_[2], m_[3]}, lv = {l_[0], l_[1], l_[2], l_[3]};
            *reinterpret_cast<u32x4*>(d + 8 * q) = hv;
            *reinterpret_cast<u32x4*>(d + PLANE + 8 * q) = mv;
            *reinterpret_cast<u32x4*>(d + 2 * PLANE + 8 * q) = lv;
        }
    }
    __syncthreads();
    const int hw = h0 + 4 * wave;                       // this wave's first image row
    const int nlive = H - hw < 4 ? H - hw : 4;          // its rows inside the image (<= 0: nothing to do; no barrier follows)
    if (nlive <= 0) return;
    f32x16 acc[4] = {zero16(), zero16(), zero16(), zero16()};
    const unsigned short* pbase = patch + ((4 * wave) * PW + li) * CP;
    // the 8 kernel values of this lane's B fragment of k-step s: kernel[(tap, c0 .. c0 + 7)][f], zeros past Cin, past the last tap, past F
    float wn[8];
    auto wload = [&](int s) {
        const int kk = 16 * s + 8 * kg, tap = kk / CP, c0 = kk % CP;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const bool ok = fok && tap < KK && c0 + i < Cin;
            wn[i] = ok ? w[(size_t)(tap * Cin + c0 + i) * F + f] : 0.f;
        }
    };
    wload(0);
    for (int s = 0; s < NS; ++s) {
        unsigned h_[4], m_[4], l_[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) split3_pair(wn[2 * i], wn[2 * i + 1], h_[i], m_[i], l_[i]);
        const u32x4 bh = {h_[0], h_[1], h_[2], h_[3]}, bm = {m_[0], m_[1], m_[2], m_[3]}, bl = {l_[0], l_[1], l_[2], l_[3]};
        if (s + 1 < NS) wload(s + 1);
        const bf16x8 wh = __builtin_bit_cast(bf16x8, bh), wm = __builtin_bit_cast(bf16x8, bm), wl = __builtin_bit_cast(bf16x8, bl);
        const int ao = tab[2 * s + kg];
        const unsigned short* pa = pbase + (ao < 0 ? 0 : ao);      // past the last tap the weights are zero: any pixel of the patch will do
        // the rows of this wave past the image read zeros of the patch; only their stores are skipped
        bf16x8 ah[4], am[4], al[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const unsigned short* ap = pa + r * PW * CP;
            ah[r] = *reinterpret_cast<const bf16x8*>(ap);
            am[r] = *reinterpret_cast<const bf16x8*>(ap + PLANE);
            al[r] = *reinterpret_cast<const bf16x8*>(ap + 2 * PLANE);
        }
        // the six products of a row in descending magnitude, the four rows interleaved (independent accumulators back to back)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = mfma_bf16(ah[r], wh, acc[r]);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = mfma_bf16(ah[r], wm, acc[r]);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = mfma_bf16(am[r], wh, acc[r]);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = mfma_bf16(ah[r], wl, acc[r]);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = mfma_bf16(al[r], wh, acc[r]);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = mfma_bf16(am[r], wm, acc[r]);
    }
    if (!fok) return;
    const float bv = bias[f];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (r < nlive) {
            float* zr = z + ((size_t)((size_t)b * H + hw + r) * W) * F + f;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int col = w0 + mfma_row(q, kg);
                if (col < W) zr[(size_t)col * F] = acc[r][q] + bv;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ Conv2D kernel / bias gradient
__global__ __launch_bounds__(256) void stem_conv_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dz, float* __restrict__ partial,
                                                              int H, int W, int Cin, int k, int F, int tilesH, int tilesW, int ntiles) {
    extern __shared__ __attribute__((aligned(16))) unsigned char stem_smem[];
    float* dzs = reinterpret_cast<float*>(stem_smem);        // [8 * 32 pixels][32 filters]
    float* patch = dzs + WG_TH * WG_TW * 32;                 // [PH][PW][Cin], then one 1.0
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kg = lane >> 5, li = lane & 31;
    const int pad = k >> 1, KK = k * k * Cin, R = KK + 1;
    const int PH = WG_TH + k - 1, PW = WG_TW + k - 1;
    const int PLANE = PH * PW * Cin;
    const int nch = (R + 31) / 32;
    const int nj = wave < nch ? (nch - wave + 3) / 4 : 0;      // this wave's chunks: wave, wave + 4, ...
    const int f = blockIdx.y * 32 + li;
    const bool fok = f < F;
    // row i of chunk j: where its patch value lies relative to the pixel's (mul 0: a constant address — the 1.0 of the bias row)
    int off[WG_MAXJ], mul[WG_MAXJ];
#pragma unroll
    for (int j = 0; j < WG_MAXJ; ++j) {
        const int i = 32 * (wave + 4 * j) + li;
        const int tap = i / Cin, c = i - tap * Cin;
        off[j] = i < KK ? ((tap / k) * PW + tap % k) * Cin + c : (i == KK ? PLANE : 0);
        mul[j] = i < KK ? 1 : 0;
    }
    f32x16 acc[WG_MAXJ];
#pragma unroll
    for (int j = 0; j < WG_MAXJ; ++j) acc[j] = zero16();
    if (tid == 0) patch[PLANE] = 1.f;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        int t = tile;
        const int tw = t % tilesW; t /= tilesW;
        const int th = t % tilesH;
        const int b = t / tilesH;
        const int h0 = th * WG_TH, w0 = tw * WG_TW;
        __syncthreads();      // the previous tile's reads are done
        for (int idx = tid; idx < PH * PW; idx += 256) {
            const int pr = idx / PW, pc = idx - pr * PW;
            const int h = h0 - pad + pr, wv = w0 - pad + pc;
            const bool ok = h >= 0 && h < H && wv >= 0 && wv < W;
            const float* p = x + (ok ? ((size_t)((size_t)b * H + h) * W + wv) * Cin : 0);
            for (int c = 0; c < Cin; ++c) patch[idx * Cin + c] = ok ? p[c] : 0.f;
        }
        // the tile's dz [256 pixels][32 filters]: zeros past the image and past F.  Staged with every load of a thread in flight at once: read from
        // global memory inside the product loop, one dependent load per step left the matrix cores waiting on memory latency
#pragma unroll 8
        for (int u = 0; u < WG_TH * WG_TW * 32 / 256; ++u) {
            const int idx = tid + 256 * u, p = idx >> 5, fl = idx & 31;
            const int h = h0 + (p >> 5), wv = w0 + (p & 31), ff = blockIdx.y * 32 + fl;
            const bool ok = ff < F && h < H && wv < W;
            dzs[idx] = ok ? dz[((size_t)((size_t)b * H + h) * W + wv) * F + ff] : 0.f;
        }
        __syncthreads();
#pragma unroll 4
        for (int step = 0; step < WG_TH * WG_TW / 2; ++step) {
            const int p = 2 * step + kg;
            const float bval = dzs[p * 32 + li];
            const int base = ((p >> 5) * PW + (p & 31)) * Cin;
#pragma unroll
            for (int j = 0; j < WG_MAXJ; ++j)
                if (j < nj) acc[j] = MFMA_F32_32x32x2(patch[base * mul[j] + off[j]], bval, acc[j]);
        }
    }
    if (!fok) return;
    float* out = partial + (size_t)blockIdx.x * R * F + f;
#pragma unroll
    for (int j = 0; j < WG_MAXJ; ++j) {
        if (j < nj) {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int i = 32 * (wave + 4 * j) + mfma_row(q, kg);
                if (i < R) out[(size_t)i * F] = acc[j][q];
            }
        }
    }
}

// dkernel [KK][F], dbias [F] = the partials [G][KK + 1][F] added in ascending order of g
__global__ __launch_bounds__(256) void stem_conv_wgrad_reduce_kernel(const float* __restrict__ partial, float* __restrict__ dkernel,
                                                                     float* __restrict__ dbias, int64_t KKF, int F, int G) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n = KKF + F;
    if (e >= n) return;
    float s = 0.f;
    for (int g = 0; g < G; ++g) s += partial[(size_t)g * n + e];
    if (e < KKF) dkernel[e] = s;
    else dbias[e - KKF] = s;
}

// ------------------------------------------------------------------------------------------------ MaxPooling2D
struct PoolGeom {
    int H, W, Ho, Wo, ph, pw, pbh, pbw;      // pb*: rows / columns of padding in front ('valid': 0)
};

__device__ __forceinline__ void take_max(float v, int pos, float& best, int& bpos, bool first) {
    const bool t = first || v > best;      // strict: the first maximum in row-major window order stays
    best = t ? v : best;
    bpos = t ? pos : bpos;
}

// VEC channels per thread (1 or 4); Cv = C / VEC
template <int VEC>
__global__ __launch_bounds__(256) void pool2d_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, unsigned char* __restrict__ idx,
                                                         int64_t total, int Cv, PoolGeom g) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int c = (int)(e % Cv);
    const int wo = (int)((e / Cv) % g.Wo), ho = (int)((e / ((int64_t)Cv * g.Wo)) % g.Ho);
    const int64_t b = e / ((int64_t)Cv * g.Wo * g.Ho);
    float best[VEC];
    int bpos[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) best[v] = 0.f, bpos[v] = 0;
    bool first = true;      // every window holds at least one in-bounds element (pad_before < p, pad_after < p)
    for (int i = 0; i < g.ph; ++i) {
        const int h = ho * g.ph - g.pbh + i;
        if (h < 0 || h >= g.H) continue;
        for (int j = 0; j < g.pw; ++j) {
            const int w = wo * g.pw - g.pbw + j;
            if (w < 0 || w >= g.W) continue;
            const size_t src = ((size_t)(b * g.H + h) * g.W + w) * Cv + c;
            if (VEC == 4) {
                const float4 q = reinterpret_cast<const float4*>(x)[src];
                take_max(q.x, i * g.pw + j, best[0], bpos[0], first);
                take_max(q.y, i * g.pw + j, best[VEC > 1 ? 1 : 0], bpos[VEC > 1 ? 1 : 0], first);
                take_max(q.z, i * g.pw + j, best[VEC > 2 ? 2 : 0], bpos[VEC > 2 ? 2 : 0], first);
                take_max(q.w, i * g.pw + j, best[VEC > 3 ? 3 : 0], bpos[VEC > 3 ? 3 : 0], first);
            } else {
                take_max(x[src], i * g.pw + j, best[0], bpos[0], first);
            }
            first = false;
        }
    }
    if (VEC == 4) {
        reinterpret_cast<float4*>(y)[e] = make_float4(best[0], best[VEC > 1 ? 1 : 0], best[VEC > 2 ? 2 : 0], best[VEC > 3 ? 3 : 0]);
        if (idx) reinterpret_cast<uchar4*>(idx)[e] = make_uchar4((unsigned char)bpos[0], (unsigned char)bpos[VEC > 1 ? 1 : 0],
                                                                 (unsigned char)bpos[VEC > 2 ? 2 : 0], (unsigned char)bpos[VEC > 3 ? 3 : 0]);
    } else {
        y[e] = best[0];
        if (idx) idx[e] = (unsigned char)bpos[0];
    }
}

// every input element lies in at most one window (strides == pool): dx = dy of that window where the element is its recorded maximum, else 0
template <int VEC>
__global__ __launch_bounds__(256) void pool2d_bwd_kernel(const float* __restrict__ dy, const unsigned char* __restrict__ idx, float* __restrict__ dx,
                                                         int64_t total, int Cv, PoolGeom g) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int c = (int)(e % Cv);
    const int w = (int)((e / Cv) % g.W), h = (int)((e / ((int64_t)Cv * g.W)) % g.H);
    const int64_t b = e / ((int64_t)Cv * g.W * g.H);
    const int hp = h + g.pbh, wp = w + g.pbw;
    const int ho = hp / g.ph, wo = wp / g.pw;
    const int pos = (hp - ho * g.ph) * g.pw + (wp - wo * g.pw);
    const bool in = ho < g.Ho && wo < g.Wo;      // 'valid' leaves the last rows / columns out
    const size_t o = in ? ((size_t)(b * g.Ho + ho) * g.Wo + wo) * Cv + c : 0;
    if (VEC == 4) {
        float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
        if (in) {
            const float4 d = reinterpret_cast<const float4*>(dy)[o];
            const uchar4 m = reinterpret_cast<const uchar4*>(idx)[o];
            r = make_float4(m.x == pos ? d.x : 0.f, m.y == pos ? d.y : 0.f, m.z == pos ? d.z : 0.f, m.w == pos ? d.w : 0.f);
        }
        reinterpret_cast<float4*>(dx)[e] = r;
    } else {
        dx[e] = (in && idx[o] == pos) ? dy[o] : 0.f;
    }
}

// SELD_OK and the geometry, or the refusal
int pool_geom(int B, int H, int W, int C, int ph, int pw, int same, PoolGeom& g) {
    if (B < 1 || H < 1 || W < 1 || C < 1 || ph < 1 || pw < 1) return SELD_ERR_INVALID;
    if ((int64_t)ph * pw > 255) return SELD_ERR_UNSUPPORTED;      // the position is a uint8
    g.H = H, g.W = W, g.ph = ph, g.pw = pw;
    if (same) {      // TensorFlow 'SAME': out = ceil(n / p), pad_total = out * p - n, pad_before = pad_total / 2
        g.Ho = (H + ph - 1) / ph, g.Wo = (W + pw - 1) / pw;
        g.pbh = (g.Ho * ph - H) / 2, g.pbw = (g.Wo * pw - W) / 2;
    } else {
        g.Ho = H / ph, g.Wo = W / pw;
        g.pbh = g.pbw = 0;
        if (g.Ho < 1 || g.Wo < 1) return SELD_ERR_INVALID;      // an empty output
    }
    return SELD_OK;
}

int stem_check(const void* a, const void* b, const void* c, const void* d, int B, int H, int W, int Cin, int k, int F) {
    if (!a || !b || !c || !d || B < 1 || H < 1 || W < 1 || Cin < 1 || k < 1 || F < 1) return SELD_ERR_INVALID;
    if (k > 7 || k % 2 == 0 || Cin > 16) return SELD_ERR_UNSUPPORTED;
    return SELD_OK;
}

int64_t stem_tiles(int B, int H, int W, int th, int tw) { return (int64_t)B * ((H + th - 1) / th) * ((W + tw - 1) / tw); }

}  // namespace

extern "C" {

int seld_stem_conv_fwd(const float* x, const float* kernel, const float* bias, float* z, int B, int H, int W, int Cin, int k, int F, void* stream) {
    const int rc = stem_check(x, kernel, bias, z, B, H, W, Cin, k, F);
    if (rc != SELD_OK) return rc;
    const int tilesH = (H + FWD_TH - 1) / FWD_TH, tilesW = (W + FWD_TW - 1) / FWD_TW;
    const int64_t ntiles = stem_tiles(B, H, W, FWD_TH, FWD_TW);
    if (ntiles > 0x7fffffff || (F + 31) / 32 > 65535) return SELD_ERR_UNSUPPORTED;
    const int CP = Cin <= 7 ? 8 : 16;
    const size_t smem = STEM_TAB * sizeof(int) + (size_t)3 * (FWD_TH + k - 1) * (FWD_TW + k - 1) * CP * sizeof(unsigned short);
    const dim3 grid((unsigned)ntiles, (unsigned)((F + 31) / 32));
    if (CP == 8) {
        hipFuncSetAttribute(reinterpret_cast<const void*>(stem_conv_fwd_kernel<8>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        hipLaunchKernelGGL(stem_conv_fwd_kernel<8>, grid, dim3(256), smem, (hipStream_t)stream, x, kernel, bias, z, H, W, Cin, k, F, tilesH, tilesW);
    } else {
        hipFuncSetAttribute(reinterpret_cast<const void*>(stem_conv_fwd_kernel<16>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        hipLaunchKernelGGL(stem_conv_fwd_kernel<16>, grid, dim3(256), smem, (hipStream_t)stream, x, kernel, bias, z, H, W, Cin, k, F, tilesH, tilesW);
    }
    return ok();
}

int64_t seld_stem_conv_wgrad_scratch(int B, int H, int W, int Cin, int k, int F) {
    if (B < 1 || H < 1 || W < 1 || Cin < 1 || k < 1 || F < 1) return SELD_ERR_INVALID;
    if (k > 7 || k % 2 == 0 || Cin > 16) return SELD_ERR_UNSUPPORTED;
    const int64_t ntiles = stem_tiles(B, H, W, WG_TH, WG_TW);
    const int64_t G = ntiles < WG_MAX_GROUPS ? ntiles : WG_MAX_GROUPS;
    return G * ((int64_t)k * k * Cin + 1) * F;
}

int seld_stem_conv_wgrad(const float* x, const float* dz, float* dkernel, float* dbias, float* scratch, int B, int H, int W, int Cin, int k, int F,
                         void* stream) {
    const int rc = stem_check(x, dz, dkernel, dbias, B, H, W, Cin, k, F);
    if (rc != SELD_OK) return rc;
    if (!scratch) return SELD_ERR_INVALID;
    const int tilesH = (H + WG_TH - 1) / WG_TH, tilesW = (W + WG_TW - 1) / WG_TW;
    const int64_t ntiles = stem_tiles(B, H, W, WG_TH, WG_TW);
    if (ntiles > 0x7fffffff || (F + 31) / 32 > 65535) return SELD_ERR_UNSUPPORTED;
    const int G = (int)(ntiles < WG_MAX_GROUPS ? ntiles : WG_MAX_GROUPS);
    const size_t smem = ((size_t)WG_TH * WG_TW * 32 + (size_t)(WG_TH + k - 1) * (WG_TW + k - 1) * Cin + 1) * sizeof(float);
    hipFuncSetAttribute(reinterpret_cast<const void*>(stem_conv_wgrad_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    hipLaunchKernelGGL(stem_conv_wgrad_kernel, dim3((unsigned)G, (unsigned)((F + 31) / 32)), dim3(256), smem, (hipStream_t)stream, x, dz, scratch, H, W,
                       Cin, k, F, tilesH, tilesW, (int)ntiles);
    const int64_t KKF = (int64_t)k * k * Cin * F;
    hipLaunchKernelGGL(stem_conv_wgrad_reduce_kernel, dim3((unsigned)((KKF + F + 255) / 256)), dim3(256), 0, (hipStream_t)stream, scratch, dkernel,
                       dbias, KKF, F, G);
    return ok();
}

int seld_pool2d_fwd(const float* x, float* y, unsigned char* idx, int B, int H, int W, int C, int ph, int pw, int same, void* stream) {
    if (!x || !y) return SELD_ERR_INVALID;
    PoolGeom g;
    const int rc = pool_geom(B, H, W, C, ph, pw, same, g);
    if (rc != SELD_OK) return rc;
    const int64_t n = (int64_t)B * g.Ho * g.Wo * C;
    if (n > (int64_t)0x7fffffff * 256) return SELD_ERR_UNSUPPORTED;
    if (C % 4 == 0 && al16(x) && al16(y) && (!idx || al4(idx)))
        hipLaunchKernelGGL(pool2d_fwd_kernel<4>, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, idx, n / 4, C / 4, g);
    else
        hipLaunchKernelGGL(pool2d_fwd_kernel<1>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, idx, n, C, g);
    return ok();
}

int seld_pool2d_bwd(const float* dy, const unsigned char* idx, float* dx, int B, int H, int W, int C, int ph, int pw, int same, void* stream) {
    if (!dy || !idx || !dx) return SELD_ERR_INVALID;
    PoolGeom g;
    const int rc = pool_geom(B, H, W, C, ph, pw, same, g);
    if (rc != SELD_OK) return rc;
    const int64_t n = (int64_t)B * H * W * C;
    if (n > (int64_t)0x7fffffff * 256) return SELD_ERR_UNSUPPORTED;
    if (C % 4 == 0 && al16(dy) && al16(dx) && al4(idx))
        hipLaunchKernelGGL(pool2d_bwd_kernel<4>, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dy, idx, dx, n / 4, C / 4, g);
    else
        hipLaunchKernelGGL(pool2d_bwd_kernel<1>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dy, idx, dx, n, C, g);
    return ok();
}

}  // extern "C"
