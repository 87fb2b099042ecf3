// vad.hip — what models.spectro_temporal_attention_based_VAD (reference models.py:105-163) needs beyond the module operators.  C ABI
// "seld_vad_*" under the seld_m_* contract (module_ops.hip): fp32 device tensors, asynchronous on the caller's stream, no allocation, no
// atomics, every sum in an order the shape alone fixes.
//
// seld_vad_gate_pool_fwd / _bwd — a * sigmoid(b) and MaxPooling2D([1, 2]) in one pass: one thread per output (forward) or input (backward)
//   element, four channels at a time where C % 4 == 0.  The gated tensor is never stored; the backward recomputes sigmoid(b) with the
//   forward's expression, so the gradient belongs to the value the forward compared.
// seld_vad_tattn_fwd / _bwd — the temporal attention.  One workgroup of 256 threads owns a clip.  Column n = d H + h: the Nt / H values of
//   head h lie H floats apart.  A (t, h) pair's sum over d is taken by G lanes of one wave (G a power of two the launcher derives from the
//   shape): lane j adds d = j, j + G, ... in ascending order, then an xor butterfly joins the G partial sums — every lane of the group adds the
//   same two numbers at each stage, so the result does not depend on the lane.  s (forward) / dP then ds (backward) live in LDS as [T][H];
//   the softmaxes over t are one thread per head (P) and per frame (score), ascending in t.
// seld_vad_bce — stage one: at most 1024 workgroups, thread i of workgroup g adds elements (g 256 + i) + j * grid in ascending j, then a
//   fixed LDS tree; stage two: one workgroup adds the partials the same way.
// seld_vad_windows / _unwindow — the irregular frame window of train_vad_baseline.py:76-106; the offset table rides in the launch.
#include "common.h"
#include "vad_win.h"

namespace {

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool al4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + __expf(-x)); }      // x -> -inf: 1 / inf = 0; x -> +inf: 1

// ------------------------------------------------------------------------------------------------ gated spectral tail
// the pair (g0, g1) of one output: y and the winner's column; the first maximum stays (seld_pool2d_fwd's take_max)
__device__ __forceinline__ float gate_max(float a0, float b0, float a1, float b1, unsigned char& pos) {
    const float g0 = a0 * sigm(b0), g1 = a1 * sigm(b1);
    const bool t = g1 > g0;
    pos = t ? 1 : 0;
    return t ? g1 : g0;
}

// VEC channels per thread (1 or 4); Cv = C / VEC, ldv = ld / VEC, Wo = W / 2
template <int VEC>
__global__ __launch_bounds__(256) void gate_pool_fwd_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ y,
                                                            unsigned char* __restrict__ idx, int64_t total, int W, int Wo, int Cv, int ldv) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int c = (int)(e % Cv);
    const int wo = (int)((e / Cv) % Wo);
    const int64_t r = e / ((int64_t)Cv * Wo);
    const size_t s0 = (size_t)(r * W + 2 * wo) * ldv + c, s1 = s0 + ldv;
    if (VEC == 4) {
        const float4 a0 = reinterpret_cast<const float4*>(a)[s0], a1 = reinterpret_cast<const float4*>(a)[s1];
        const float4 b0 = reinterpret_cast<const float4*>(b)[s0], b1 = reinterpret_cast<const float4*>(b)[s1];
        uchar4 p;
        float4 o;
        o.x = gate_max(a0.x, b0.x, a1.x, b1.x, p.x);
        o.y = gate_max(a0.y, b0.y, a1.y, b1.y, p.y);
        o.z = gate_max(a0.z, b0.z, a1.z, b1.z, p.z);
        o.w = gate_max(a0.w, b0.w, a1.w, b1.w, p.w);
        reinterpret_cast<float4*>(y)[e] = o;
        if (idx) reinterpret_cast<uchar4*>(idx)[e] = p;
    } else {
        unsigned char p;
        y[e] = gate_max(a[s0], b[s0], a[s1], b[s1], p);
        if (idx) idx[e] = p;
    }
}

// d = the pooled gradient that reaches this element (0 at a loser): da = d s, db = d a s (1 - s)
__device__ __forceinline__ void gate_grad(float a, float b, float d, bool win, float& da, float& db) {
    const float s = sigm(b);
    da = win ? d * s : 0.f;
    db = win ? d * a * (s * (1.f - s)) : 0.f;
}

template <int VEC>
__global__ __launch_bounds__(256) void gate_pool_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                            const unsigned char* __restrict__ idx, const float* __restrict__ dy,
                                                            float* __restrict__ da, float* __restrict__ db, int64_t total, int W, int Wo, int Cv,
                                                            int ldv) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;      // over [rows][W][Cv]
    if (e >= total) return;
    const int c = (int)(e % Cv);
    const int w = (int)((e / Cv) % W);
    const int64_t r = e / ((int64_t)Cv * W);
    const int wo = w >> 1;
    const unsigned char side = (unsigned char)(w & 1);
    const bool in = wo < Wo;      // 'valid' leaves an odd last column out
    const size_t src = (size_t)(r * W + w) * ldv + c;
    const size_t o = in ? (size_t)(r * Wo + wo) * Cv + c : 0;
    if (VEC == 4) {
        float4 ra = make_float4(0.f, 0.f, 0.f, 0.f), rb = ra;
        if (in) {
            const float4 d = reinterpret_cast<const float4*>(dy)[o];
            const uchar4 m = reinterpret_cast<const uchar4*>(idx)[o];
            const float4 av = reinterpret_cast<const float4*>(a)[src], bv = reinterpret_cast<const float4*>(b)[src];
            gate_grad(av.x, bv.x, d.x, m.x == side, ra.x, rb.x);
            gate_grad(av.y, bv.y, d.y, m.y == side, ra.y, rb.y);
            gate_grad(av.z, bv.z, d.z, m.z == side, ra.z, rb.z);
            gate_grad(av.w, bv.w, d.w, m.w == side, ra.w, rb.w);
        }
        reinterpret_cast<float4*>(da)[src] = ra;
        reinterpret_cast<float4*>(db)[src] = rb;
    } else {
        float ra = 0.f, rb = 0.f;
        if (in) gate_grad(a[src], b[src], dy[o], idx[o] == side, ra, rb);
        da[src] = ra;
        db[src] = rb;
    }
}

int gate_pool_check(const void* a, const void* b, int ld, int64_t rows, int W, int C) {
    if (!a || !b || rows < 1 || W < 2 || C < 1 || ld < C) return SELD_ERR_INVALID;
    if (rows > (int64_t)0x7fffffff * 256 / ((int64_t)W * C)) return SELD_ERR_UNSUPPORTED;      // the grid: elements / 256 workgroups in 31 bits
    return SELD_OK;
}

// ------------------------------------------------------------------------------------------------ temporal attention
constexpr int TA_THREADS = 256;

// lanes that share one (t, h) pair's sum over d: a power of two <= 64, no more than D, enough that the pairs fill the workgroup
int tattn_group(int T, int H, int D) {
    int G = 1;
    while (G < 64 && G * 2 <= D && (int64_t)T * H * G < TA_THREADS) G *= 2;
    return G;
}
size_t tattn_smem(int T, int Nt, int H) { return ((size_t)Nt + (size_t)T * H + (size_t)T) * sizeof(float); }

// sum over d of x[d H + h] sigmoid(y[d H + h]), taken by the G lanes j = 0 .. G - 1 of a group.  Every lane of the wave calls it (the lanes of
// a pair past the end pass valid = false and add nothing)
__device__ __forceinline__ float head_dot(const float* __restrict__ x, const float* __restrict__ y, int h, int H, int D, int G, int j, bool valid) {
    float acc = 0.f;
    if (valid)
        for (int d = j; d < D; d += G) acc = fmaf(x[d * H + h], sigm(y[d * H + h]), acc);
    for (int o = G >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    return acc;
}

__global__ __launch_bounds__(TA_THREADS) void tattn_fwd_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                               float* __restrict__ y, float* __restrict__ score, float* __restrict__ P, int T, int Nt,
                                                               int H, int G, float c) {
    extern __shared__ __attribute__((aligned(16))) float ta_smem[];
    float* sq = ta_smem;              // [Nt] sigmoid(q)
    float* s = sq + Nt;               // [T][H] logits, then P
    float* ssum = s + T * H;          // [T] sum_h s
    const int tid = threadIdx.x, D = Nt / H;
    const size_t b = blockIdx.x;
    q += b * Nt, k += b * T * Nt, v += b * T * Nt, y += b * T * Nt, score += b * T;
    for (int n = tid; n < Nt; n += TA_THREADS) sq[n] = sigm(q[n]);
    __syncthreads();
    const int npair = T * H, per = TA_THREADS / G, j = tid & (G - 1);
    for (int p0 = 0; p0 < npair; p0 += per) {
        const int p = p0 + tid / G;
        const bool valid = p < npair;
        const int t = valid ? p / H : 0, h = valid ? p - t * H : 0;
        const float acc = head_dot(sq, k + (size_t)t * Nt, h, H, D, G, j, valid);
        if (valid && j == 0) s[p] = c * acc;
    }
    __syncthreads();
    for (int t = tid; t < T; t += TA_THREADS) {
        float a = 0.f;
        for (int h = 0; h < H; ++h) a += s[t * H + h];
        ssum[t] = a;
    }
    __syncthreads();
    for (int t = tid; t < T; t += TA_THREADS) {      // softmax over t of ssum: every thread walks the T values in the same order
        float m = ssum[0];
        for (int u = 1; u < T; ++u) m = fmaxf(m, ssum[u]);
        float z = 0.f;
        for (int u = 0; u < T; ++u) z += __expf(ssum[u] - m);
        score[t] = __expf(ssum[t] - m) / z;
    }
    for (int h = tid; h < H; h += TA_THREADS) {      // softmax over t per head, in place
        float m = s[h];
        for (int t = 1; t < T; ++t) m = fmaxf(m, s[t * H + h]);
        float z = 0.f;
        for (int t = 0; t < T; ++t) z += __expf(s[t * H + h] - m);
        for (int t = 0; t < T; ++t) {
            const float pv = __expf(s[t * H + h] - m) / z;
            s[t * H + h] = pv;
            if (P) P[(b * T + t) * H + h] = pv;
        }
    }
    __syncthreads();
    for (int e = tid; e < T * Nt; e += TA_THREADS) {
        const int t = e / Nt, n = e - t * Nt;
        y[e] = sigm(v[e]) * s[t * H + n % H];
    }
}

__global__ __launch_bounds__(TA_THREADS) void tattn_bwd_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                               const float* __restrict__ P, const float* __restrict__ score,
                                                               const float* __restrict__ dy, const float* __restrict__ dscore, float* __restrict__ dq,
                                                               float* __restrict__ dk, float* __restrict__ dv, int T, int Nt, int H, int G, float c) {
    extern __shared__ __attribute__((aligned(16))) float ta_smem[];
    float* sq = ta_smem;              // [Nt] sigmoid(q)
    float* ds = sq + Nt;              // [T][H] dP, then ds
    float* dS = ds + T * H;           // [T]
    const int tid = threadIdx.x, D = Nt / H;
    const size_t b = blockIdx.x;
    q += b * Nt, dq += b * Nt, k += b * T * Nt, v += b * T * Nt, dy += b * T * Nt, dk += b * T * Nt, dv += b * T * Nt;
    P += b * T * H, score += b * T, dscore += b * T;
    for (int n = tid; n < Nt; n += TA_THREADS) sq[n] = sigm(q[n]);
    const int npair = T * H, per = TA_THREADS / G, j = tid & (G - 1);
    for (int p0 = 0; p0 < npair; p0 += per) {      // dP[t,h] = sum_d dy sigmoid(v)
        const int p = p0 + tid / G;
        const bool valid = p < npair;
        const int t = valid ? p / H : 0, h = valid ? p - t * H : 0;
        const float acc = head_dot(dy + (size_t)t * Nt, v + (size_t)t * Nt, h, H, D, G, j, valid);
        if (valid && j == 0) ds[p] = acc;
    }
    for (int t = tid; t < T; t += TA_THREADS) {
        float dot = 0.f;
        for (int u = 0; u < T; ++u) dot = fmaf(score[u], dscore[u], dot);
        dS[t] = score[t] * (dscore[t] - dot);
    }
    __syncthreads();
    for (int h = tid; h < H; h += TA_THREADS) {
        float dot = 0.f;
        for (int t = 0; t < T; ++t) dot = fmaf(P[t * H + h], ds[t * H + h], dot);
        for (int t = 0; t < T; ++t) ds[t * H + h] = P[t * H + h] * (ds[t * H + h] - dot) + dS[t];
    }
    __syncthreads();
    for (int n = tid; n < Nt; n += TA_THREADS) {      // a thread owns a column: dv, dk of its T elements and dq's sum over t, ascending
        const int h = n % H;
        const float qs = sq[n];
        float acc = 0.f;
        for (int t = 0; t < T; ++t) {
            const size_t e = (size_t)t * Nt + n;
            const float vs = sigm(v[e]), ks = sigm(k[e]), g = ds[t * H + h];
            dv[e] = dy[e] * P[t * H + h] * (vs * (1.f - vs));
            dk[e] = c * g * qs * (ks * (1.f - ks));
            acc = fmaf(g, ks, acc);
        }
        dq[n] = c * acc * (qs * (1.f - qs));
    }
}

int tattn_check(int B, int T, int Nt, int H) {
    if (B < 1 || T < 1 || Nt < 1 || H < 1 || H > Nt || Nt % H) return SELD_ERR_INVALID;
    if (Nt > SELD_VAD_MAX_NT || T > SELD_VAD_MAX_T) return SELD_ERR_UNSUPPORTED;
    return SELD_OK;
}

// ------------------------------------------------------------------------------------------------ binary cross-entropy
constexpr int BCE_MAX_BLOCKS = 1024;
constexpr float BCE_EPS = 1e-7f;

int bce_blocks(int64_t n) {
    const int64_t g = (n + 255) / 256;
    return (int)(g < BCE_MAX_BLOCKS ? g : BCE_MAX_BLOCKS);
}

// the workgroup's 256 values -> their sum in thread 0, by a fixed tree
__device__ __forceinline__ float block_sum256(float v, float* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(256) void bce_partial_kernel(const float* __restrict__ p, const float* __restrict__ y, float* __restrict__ dp,
                                                          float* __restrict__ partial, int64_t n, float gscale) {
    __shared__ float red[256];
    const int64_t stride = (int64_t)gridDim.x * 256;
    const float lo = BCE_EPS, hi = 1.f - BCE_EPS;
    float acc = 0.f;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += stride) {
        const float pv = p[e], yv = y[e];
        const float pc = fminf(fmaxf(pv, lo), hi);
        const float u = pc + BCE_EPS, w = 1.f - pc + BCE_EPS;
        acc -= yv * logf(u) + (1.f - yv) * logf(w);
        if (dp) dp[e] = (pv < lo || pv > hi) ? 0.f : gscale * ((1.f - yv) / w - yv / u);
    }
    const float tot = block_sum256(acc, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

__global__ __launch_bounds__(256) void bce_final_kernel(const float* __restrict__ partial, int nblk, float* __restrict__ loss, float scale,
                                                        int accumulate) {
    __shared__ float red[256];
    float acc = 0.f;
    for (int i = threadIdx.x; i < nblk; i += 256) acc += partial[i];
    const float tot = block_sum256(acc, red);
    if (threadIdx.x == 0) *loss = (accumulate ? *loss : 0.f) + scale * tot;
}

// ------------------------------------------------------------------------------------------------ frame windows
__global__ __launch_bounds__(256) void vad_windows_kernel(const float* __restrict__ x, float* __restrict__ win, int64_t total, int D, WinTable tb) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;      // over [n_windows][Wn][D]
    if (e >= total) return;
    const int d = (int)(e % D);
    const int i = (int)((e / D) % tb.n);
    const int64_t n = e / ((int64_t)D * tb.n);
    win[e] = x[(n + tb.offs[i]) * D + d];
}

__global__ __launch_bounds__(256) void vad_unwindow_kernel(const float* __restrict__ win, float* __restrict__ seq, int64_t total, int64_t n_windows,
                                                           int D, WinTable tb) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;      // over [n_windows + width][D]
    if (e >= total) return;
    const int d = (int)(e % D);
    const int64_t m = e / D;
    float acc = 0.f, cnt = 0.f;
    for (int i = 0; i < tb.n; ++i) {
        const int64_t n = m - tb.offs[i];
        if (n < 0 || n >= n_windows) continue;
        acc += win[(n * tb.n + i) * D + d];
        cnt += 1.f;
    }
    seq[e] = acc / (cnt + 1e-8f);
}

}  // namespace

extern "C" {

int seld_vad_gate_pool_fwd(const float* a, const float* b, int ld, float* y, unsigned char* idx, int64_t rows, int W, int C, void* stream) {
    if (!y) return SELD_ERR_INVALID;
    const int rc = gate_pool_check(a, b, ld, rows, W, C);
    if (rc != SELD_OK) return rc;
    const int Wo = W / 2;
    const int64_t n = rows * Wo * C;
    if (C % 4 == 0 && ld % 4 == 0 && al16(a) && al16(b) && al16(y) && (!idx || al4(idx)))
        hipLaunchKernelGGL(gate_pool_fwd_kernel<4>, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, b, y, idx, n / 4, W, Wo,
                           C / 4, ld / 4);
    else
        hipLaunchKernelGGL(gate_pool_fwd_kernel<1>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, b, y, idx, n, W, Wo, C, ld);
    return ok();
}

int seld_vad_gate_pool_bwd(const float* a, const float* b, int ld, const unsigned char* idx, const float* dy, float* da, float* db, int64_t rows,
                           int W, int C, void* stream) {
    if (!idx || !dy || !da || !db) return SELD_ERR_INVALID;
    const int rc = gate_pool_check(a, b, ld, rows, W, C);
    if (rc != SELD_OK) return rc;
    const int Wo = W / 2;
    const int64_t n = rows * W * C;
    if (C % 4 == 0 && ld % 4 == 0 && al16(a) && al16(b) && al16(dy) && al16(da) && al16(db) && al4(idx))
        hipLaunchKernelGGL(gate_pool_bwd_kernel<4>, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, b, idx, dy, da, db,
                           n / 4, W, Wo, C / 4, ld / 4);
    else
        hipLaunchKernelGGL(gate_pool_bwd_kernel<1>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, b, idx, dy, da, db, n, W,
                           Wo, C, ld);
    return ok();
}

int seld_vad_tattn_fwd(const float* q, const float* k, const float* v, float* y, float* score, float* P, int B, int T, int Nt, int H, void* stream) {
    if (!q || !k || !v || !y || !score) return SELD_ERR_INVALID;
    const int rc = tattn_check(B, T, Nt, H);
    if (rc != SELD_OK) return rc;
    const size_t smem = tattn_smem(T, Nt, H);
    if (smem > 64 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(tattn_fwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) != hipSuccess)
        return SELD_ERR_HIP;
    hipLaunchKernelGGL(tattn_fwd_kernel, dim3((unsigned)B), dim3(TA_THREADS), smem, (hipStream_t)stream, q, k, v, y, score, P, T, Nt, H,
                       tattn_group(T, H, Nt / H), 1.f / sqrtf((float)Nt));
    return ok();
}

int seld_vad_tattn_bwd(const float* q, const float* k, const float* v, const float* P, const float* score, const float* dy, const float* dscore,
                       float* dq, float* dk, float* dv, int B, int T, int Nt, int H, void* stream) {
    if (!q || !k || !v || !P || !score || !dy || !dscore || !dq || !dk || !dv) return SELD_ERR_INVALID;
    const int rc = tattn_check(B, T, Nt, H);
    if (rc != SELD_OK) return rc;
    const size_t smem = tattn_smem(T, Nt, H);
    if (smem > 64 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(tattn_bwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) != hipSuccess)
        return SELD_ERR_HIP;
    hipLaunchKernelGGL(tattn_bwd_kernel, dim3((unsigned)B), dim3(TA_THREADS), smem, (hipStream_t)stream, q, k, v, P, score, dy, dscore, dq, dk, dv, T,
                       Nt, H, tattn_group(T, H, Nt / H), 1.f / sqrtf((float)Nt));
    return ok();
}

int64_t seld_vad_bce_scratch(int64_t n) { return n > 0 ? (int64_t)bce_blocks(n) : -1; }

int seld_vad_bce(const float* p, const float* y, float* loss, float* dp, float* scratch, int64_t n, float weight, int accumulate, void* stream) {
    if (!p || !y || !loss || !scratch || n < 1) return SELD_ERR_INVALID;
    const int nblk = bce_blocks(n);
    const float scale = (float)((double)weight / (double)n);
    hipLaunchKernelGGL(bce_partial_kernel, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, p, y, dp, scratch, n, scale);
    hipLaunchKernelGGL(bce_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, scratch, nblk, loss, scale, accumulate);
    return ok();
}

int seld_vad_windows(const float* x, float* win, const int32_t* offs, int Wn, int64_t len, int D, void* stream) {
    if (!x || !win || len < 1 || D < 1) return SELD_ERR_INVALID;
    WinTable tb;
    const int rc = win_table(offs, Wn, tb);
    if (rc != SELD_OK) return rc;
    if (len <= tb.width) return SELD_ERR_INVALID;      // no window fits
    const int64_t total = (len - tb.width) * Wn * D;
    if (total > (int64_t)0x7fffffff * 256) return SELD_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(vad_windows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, win, total, D, tb);
    return ok();
}

int seld_vad_unwindow(const float* win, float* seq, const int32_t* offs, int Wn, int64_t n_windows, int D, void* stream) {
    if (!win || !seq || n_windows < 1 || D < 1) return SELD_ERR_INVALID;
    WinTable tb;
    const int rc = win_table(offs, Wn, tb);
    if (rc != SELD_OK) return rc;
    const int64_t total = (n_windows + tb.width) * D;
    if (total > (int64_t)0x7fffffff * 256 || n_windows * Wn > (int64_t)0x7fffffff * 256 / D) return SELD_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(vad_unwindow_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, win, seq, total, n_windows, D, tb);
    return ok();
}

}  // extern "C"
