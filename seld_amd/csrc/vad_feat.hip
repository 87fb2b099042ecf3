// vad_feat.hip — the data path of the voice-activity task (reference vad_dataloader.py:77-136, train_vad_baseline.py:49, 216-224): the
// log-mel front end of tf.signal.stft + linear_to_mel_weight_matrix, sample labels -> frame labels, the random-window batch gather and the
// threshold counters behind AUC / Precision / Recall.  C ABI "seld_vad_*" under the seld_m_* contract (module_ops.hip): fp32 device tensors,
// asynchronous on the caller's stream, no allocation after create, no host synchronisation.  Every device read is bounded by the totals the
// caller passes as host scalars: a wrong table gives wrong values, never an out-of-range access.
//
// seld_vad_feat_extract — a packed corpus (utterances end to end) in two launches.
//   vad_feat_kernel: one WAVE per frame, persistent, tables shared in LDS.  The frame is NOT centred or padded (tf.signal.stft): frame j of a
//   file starts at sample j n_fft / 2.  Periodic Hann, then the real transform by the half-length trick: even and odd windowed samples are the
//   real and imaginary parts of an n_fft / 2 point complex transform (wave_fft.h, fp32), one split pass with the n_fft-point twiddles gives
//   bins 0 .. n_fft / 2.  A frame's values therefore depend on that frame's samples alone.  |X| goes to the wave's LDS plane, lane m + 64 i
//   adds filter m's contiguous bin range in ascending order (an empty range: exactly 0) and the row is stored raw.
//   vad_feat_post_kernel: one workgroup per file: minimum and maximum of the file's raw rows, then log(min(max(s, 1e-8), M)) and
//   (v - min) / (max - min) in place with the arithmetic written literally — a silent file comes out all NaN, as the reference's does.  The
//   log is monotone, so the logged extrema are the logs of the raw ones: one read pass, one write pass, no atomics, no partial buffers.
// seld_vad_frame_labels — one wave per frame: lane l adds samples l, l + 64, ... in ascending order, an xor butterfly joins the 64 sums
//   (every lane adds the same two numbers at each stage), rintf(sum / n_fft) is tf.round's half-to-even.
// seld_vad_gather — one thread per output element; the window's offset table rides in the launch, rows are clamped into the corpus.
// seld_vad_score_update — threshold buckets in a workgroup's LDS (32-bit integer atomics), then one 64-bit integer atomic per non-empty
//   bucket and workgroup: integers, so exact in any order.
#include "common.h"
#include "vad_win.h"
#include "wave_fft.h"

#include <math.h>
#include <vector>

struct seld_vadfeat {
    int device = 0, sample_rate = 0, n_fft = 0, n_mels = 0;
    int n_melw = 0;             // floats of the sparse filter table
    float* win = nullptr;       // [n_fft] periodic Hann
    float2* tw_half = nullptr;  // [n_fft / 4]: exp(-2 pi i t / (n_fft / 2)), the complex transform's
    float2* tw_full = nullptr;  // [n_fft / 2]: exp(-2 pi i k / n_fft), the split pass's
    int* mel_start = nullptr;   // [n_mels] first bin | bins | offset into mel_w
    int* mel_cnt = nullptr;
    int* mel_off = nullptr;
    float* mel_w = nullptr;
};

namespace {

constexpr int VF_WAVES = 8;
constexpr float VF_FLOOR = 1e-8f;      // vad_dataloader.py:92

// the file of global frame t: the largest f in [0, n_files) with frame_starts[f] <= t (every index read lies in [0, n_files))
__device__ __forceinline__ int file_of(const int64_t* __restrict__ frame_starts, int n_files, int64_t t) {
    int lo = 0, hi = n_files - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (frame_starts[mid] <= t) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// first sample of global frame t, clamped so that [s0, s0 + n_fft) lies in [0, total_samples) whatever the tables hold
__device__ __forceinline__ int64_t frame_sample0(const int64_t* __restrict__ sample_starts, const int64_t* __restrict__ frame_starts, int n_files,
                                                 int64_t t, int n_fft, int64_t total_samples) {
    const int f = file_of(frame_starts, n_files, t);
    int64_t s0 = sample_starts[f] + (t - frame_starts[f]) * (n_fft / 2);
    if (s0 > total_samples - n_fft) s0 = total_samples - n_fft;
    if (s0 < 0) s0 = 0;
    return s0;
}

static size_t vf_wave_bytes(int n_fft) { return (size_t)(n_fft / 2) * sizeof(float2); }
static size_t vf_smem(int n_fft, int n_mels, int n_melw) {
    // tw_half | tw_full | win | mel_w (padded to 4 floats) | start, cnt, off (each padded to 4 ints) | VF_WAVES transform buffers
    return (size_t)(n_fft / 4) * 8 + (size_t)(n_fft / 2) * 8 + (size_t)n_fft * 4 + (size_t)((n_melw + 3) & ~3) * 4 + (size_t)3 * ((n_mels + 3) & ~3) * 4 +
           VF_WAVES * vf_wave_bytes(n_fft);
}

template <int LOGM>      // M = n_fft / 2 = 1 << LOGM complex points
__global__ __launch_bounds__(64 * VF_WAVES) void vad_feat_kernel(
    const float* __restrict__ wav, const int64_t* __restrict__ sample_starts, const int64_t* __restrict__ frame_starts, int n_files,
    int64_t total_samples, int64_t total_frames, int n_mels, int n_melw, const float* __restrict__ win_g, const float2* __restrict__ twh_g,
    const float2* __restrict__ twf_g, const int* __restrict__ mel_start, const int* __restrict__ mel_cnt, const int* __restrict__ mel_off,
    const float* __restrict__ mel_w, float* __restrict__ out) {
    using G = WF<LOGM>;
    constexpr int M = G::N, N = 2 * M, NB4 = G::NB4, Q = M / 4;
    constexpr int NBI = M / 64 + 1;                                // bins 0 .. M per lane
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float2* twh = reinterpret_cast<float2*>(smem);                 // [M / 2]
    float2* twf = twh + M / 2;                                     // [M]
    float* win = reinterpret_cast<float*>(twf + M);                // [N]
    float* melw = win + N;                                         // [n_melw]
    const int nmp = (n_mels + 3) & ~3;
    int* mst = reinterpret_cast<int*>(melw + ((n_melw + 3) & ~3));
    int* mct = mst + nmp;
    int* mof = mct + nmp;
    const int tid = threadIdx.x, lane_id = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float2* buf = reinterpret_cast<float2*>(mof + nmp) + (size_t)wave * M;
    float* val = reinterpret_cast<float*>(buf);                    // the same bytes later hold |X| of bins 0 .. M (2 M floats >= M + 1)
    for (int i = tid; i < M / 2; i += 64 * VF_WAVES) twh[i] = twh_g[i];
    for (int i = tid; i < M; i += 64 * VF_WAVES) twf[i] = twf_g[i];
    for (int i = tid; i < N; i += 64 * VF_WAVES) win[i] = win_g[i];
    for (int i = tid; i < n_melw; i += 64 * VF_WAVES) melw[i] = mel_w[i];
    for (int i = tid; i < n_mels; i += 64 * VF_WAVES) { mst[i] = mel_start[i]; mct[i] = mel_cnt[i]; mof[i] = mel_off[i]; }
    __syncthreads();
    float2* const b1[1] = {buf};
    for (int64_t t = (int64_t)blockIdx.x * VF_WAVES + wave; t < total_frames; t += (int64_t)gridDim.x * VF_WAVES) {
        // `lane` made opaque per frame: what it indexes (twiddles of every pass, window) is otherwise hoisted out of this loop and held in
        // registers for the one or two frames a wave sees (features.hip's feat_wave_kernel)
        int lane = lane_id;
        asm volatile("" : "+v"(lane));
        const float* p = wav + frame_sample0(sample_starts, frame_starts, n_files, t, N, total_samples);
        float2 v[1][NB4][4];
#pragma unroll
        for (int b = 0; b < NB4; ++b)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int n = lane + 64 * b + q * Q;               // complex element n = samples 2 n, 2 n + 1
                const float2 w = reinterpret_cast<const float2*>(win)[n];
                v[0][b][q] = make_float2(w.x * p[2 * n], w.y * p[2 * n + 1]);
            }
        wave_fft<LOGM, 1, true>(v, b1, twh, lane);
        // X[k] = E[k] + W^k O[k], E = (Z[k] + conj(Z[M-k])) / 2, O = (Z[k] - conj(Z[M-k])) / (2 i), W = exp(-2 pi i / N); Z[M] = Z[0], W^M = -1
        float mag[NBI];
#pragma unroll
        for (int i = 0; i < NBI; ++i) {
            const int k = lane + 64 * i, kk = k <= M ? k : 0;
            const float2 a = buf[kk & (M - 1)], c = buf[(M - kk) & (M - 1)];
            const float2 e = make_float2(0.5f * (a.x + c.x), 0.5f * (a.y - c.y));
            const float2 o = make_float2(0.5f * (a.y + c.y), 0.5f * (c.x - a.x));
            const float2 w = kk < M ? twf[kk] : make_float2(-1.f, 0.f);
            const float2 wo = cmul(w, o);
            const float re = e.x + wo.x, im = e.y + wo.y;
            mag[i] = sqrtf(re * re + im * im);
        }
        WAVE_LDS_FENCE();        // every bin is in registers before the plane overwrites the transform
#pragma unroll
        for (int i = 0; i < NBI; ++i) {
            const int k = lane + 64 * i;
            if (k <= M) val[k] = mag[i];
        }
        WAVE_LDS_FENCE();
        float* row = out + t * n_mels;
        for (int m = lane; m < n_mels; m += 64) {
            const float* wv = melw + mof[m];
            const float* vv = val + mst[m];
            const int cnt = mct[m];
            float acc = 0.f;
            for (int j = 0; j < cnt; ++j) acc = fmaf(vv[j], wv[j], acc);
            row[m] = acc;
        }
        WAVE_LDS_FENCE();        // the plane is read before the next frame's first pass writes the buffer
    }
}

// tf.clip_by_value(s, 1e-8, mx) then log, written as the reference computes it: min(max(s, lo), hi) — with hi < lo the result is hi
__device__ __forceinline__ float vf_log(float s, float mx) {
    float c = s < VF_FLOOR ? VF_FLOOR : s;
    c = c > mx ? mx : c;
    return logf(c);
}

__global__ __launch_bounds__(256) void vad_feat_post_kernel(float* __restrict__ out, const int64_t* __restrict__ frame_starts, int64_t total_frames,
                                                            int n_mels, int logmel, int normalize) {
    __shared__ float rmin[256], rmax[256];
    const int f = blockIdx.x, tid = threadIdx.x;
    int64_t r0 = frame_starts[f], r1 = frame_starts[f + 1];
    r0 = r0 < 0 ? 0 : (r0 > total_frames ? total_frames : r0);
    r1 = r1 < r0 ? r0 : (r1 > total_frames ? total_frames : r1);
    float* x = out + r0 * n_mels;
    const int64_t n = (r1 - r0) * n_mels;
    float lo = INFINITY, hi = -INFINITY;
    for (int64_t i = tid; i < n; i += 256) {
        const float s = x[i];
        lo = fminf(lo, s);
        hi = fmaxf(hi, s);
    }
    rmin[tid] = lo, rmax[tid] = hi;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) { rmin[tid] = fminf(rmin[tid], rmin[tid + w]); rmax[tid] = fmaxf(rmax[tid], rmax[tid + w]); }
        __syncthreads();
    }
    const float smin = rmin[0], smax = rmax[0];
    // the extrema of the logged values are the logged raw extrema (log and the clip are monotone)
    const float vmin = logmel ? vf_log(smin, smax) : smin, vmax = logmel ? vf_log(smax, smax) : smax;
    const float range = vmax - vmin;
    for (int64_t i = tid; i < n; i += 256) {
        float v = x[i];
        if (logmel) v = vf_log(v, smax);
        if (normalize) v = (v - vmin) / range;
        x[i] = v;
    }
}

__global__ __launch_bounds__(256) void vad_frame_labels_kernel(const float* __restrict__ labels, const int64_t* __restrict__ sample_starts,
                                                               const int64_t* __restrict__ frame_starts, int n_files, int64_t total_samples,
                                                               int64_t total_frames, int n_fft, float* __restrict__ y) {
    const int lane = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= total_frames) return;
    const float* p = labels + frame_sample0(sample_starts, frame_starts, n_files, t, n_fft, total_samples);
    float acc = 0.f;
    for (int i = lane; i < n_fft; i += 64) acc += p[i];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) y[t] = rintf(acc / (float)n_fft);
}

__global__ __launch_bounds__(256) void vad_gather_kernel(const float* __restrict__ feat, const float* __restrict__ y, const int64_t* __restrict__ pos,
                                                         int64_t total, int D, int64_t total_frames, float* __restrict__ x_out,
                                                         float* __restrict__ y_out, WinTable tb) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;      // over [B][Wn][D]
    if (e >= total) return;
    const int d = (int)(e % D);
    const int64_t bi = e / D;
    int64_t r = pos[bi / tb.n] + tb.offs[(int)(bi % tb.n)];
    r = r < 0 ? 0 : (r >= total_frames ? total_frames - 1 : r);
    x_out[e] = feat[r * D + d];
    if (d == 0) y_out[bi] = y[r];
}

#define SCORE_MAX_NT 1024
__global__ __launch_bounds__(256) void vad_score_kernel(const float* __restrict__ pred, const float* __restrict__ y, int64_t n,
                                                        const float* __restrict__ thresholds, int NT, unsigned long long* __restrict__ counts) {
    __shared__ float thr[SCORE_MAX_NT];
    __shared__ unsigned int cnt[2 * (SCORE_MAX_NT + 1)];
    const int tid = threadIdx.x;
    for (int i = tid; i < NT; i += 256) thr[i] = thresholds[i];
    for (int i = tid; i < 2 * (NT + 1); i += 256) cnt[i] = 0u;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < n; i += (int64_t)gridDim.x * 256) {
        const float p = pred[i];
        int lo = 0, hi = NT;      // the number of thresholds below p: a NaN compares false everywhere and lands in bucket 0
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (p > thr[mid]) lo = mid + 1; else hi = mid;
        }
        atomicAdd(&cnt[2 * lo + (y[i] != 0.f ? 1 : 0)], 1u);
    }
    __syncthreads();
    for (int i = tid; i < 2 * (NT + 1); i += 256)
        if (cnt[i]) atomicAdd(&counts[i], (unsigned long long)cnt[i]);
}

double hz_to_mel(double f) { return 1127.0 * log(1.0 + f / 700.0); }

int mel_matrix(int n_mels, int n_bins, int sample_rate, double lower_hz, double upper_hz, float* w) {
    if (!w || n_mels < 1 || n_bins < 2 || sample_rate < 1 || !(lower_hz >= 0.0) || !(lower_hz < upper_hz) || !(upper_hz <= sample_rate / 2.0))
        return SELD_ERR_INVALID;
    const double m_lo = hz_to_mel(lower_hz), m_hi = hz_to_mel(upper_hz), nyq = sample_rate / 2.0;
    std::vector<double> edge(n_mels + 2);
    for (int j = 0; j < n_mels + 2; ++j) edge[j] = m_lo + (m_hi - m_lo) * j / (n_mels + 1);
    for (int k = 0; k < n_bins; ++k) {
        const double mk = hz_to_mel(nyq * k / (n_bins - 1));
        for (int m = 0; m < n_mels; ++m) {
            const double up = (mk - edge[m]) / (edge[m + 1] - edge[m]), down = (edge[m + 2] - mk) / (edge[m + 2] - edge[m + 1]);
            const double v = up < down ? up : down;
            w[(size_t)k * n_mels + m] = k == 0 || !(v > 0.0) ? 0.f : (float)v;      // row 0 (DC) is zero whatever the lower edge
        }
    }
    return SELD_OK;
}

int logm_of(int n_fft) { return n_fft == 512 ? 8 : n_fft == 1024 ? 9 : n_fft == 2048 ? 10 : 0; }

}  // namespace

extern "C" {

int64_t seld_vad_feat_frames(int n_fft, int64_t n_samples) {
    if (n_fft < 2 || n_samples < n_fft) return 0;
    return 1 + (n_samples - n_fft) / (n_fft / 2);
}

int seld_vad_mel_matrix_host(int n_mels, int n_bins, int sample_rate, double lower_hz, double upper_hz, float* w) {
    return mel_matrix(n_mels, n_bins, sample_rate, lower_hz, upper_hz, w);
}

void seld_vad_feat_destroy(seld_vadfeat* f) {
    if (!f) return;
    hipFree(f->win); hipFree(f->tw_half); hipFree(f->tw_full);
    hipFree(f->mel_start); hipFree(f->mel_cnt); hipFree(f->mel_off); hipFree(f->mel_w);
    delete f;
}

int seld_vad_feat_create(int sample_rate, int n_fft, int n_mels, int device, seld_vadfeat** out) {
    if (!out) return SELD_ERR_INVALID;
    *out = nullptr;
    if (sample_rate < 2 || n_fft < 2 || n_mels < 1 || device < 0) return SELD_ERR_INVALID;
    if (!logm_of(n_fft) || n_mels > SELD_VAD_MAX_MELS) return SELD_ERR_UNSUPPORTED;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device >= ndev) return SELD_ERR_HIP;
    const int M = n_fft / 2, n_bins = M + 1;
    const double PI = 3.14159265358979323846;
    std::vector<float> win(n_fft), dense((size_t)n_bins * n_mels), mw;
    std::vector<float2> twh(M / 2), twf(M);
    for (int n = 0; n < n_fft; ++n) win[n] = (float)(0.5 - 0.5 * cos(2.0 * PI * n / n_fft));      // tf.signal.hann_window(periodic=True)
    for (int t = 0; t < M / 2; ++t) twh[t] = make_float2((float)cos(2.0 * PI * t / M), (float)-sin(2.0 * PI * t / M));
    for (int k = 0; k < M; ++k) twf[k] = make_float2((float)cos(2.0 * PI * k / n_fft), (float)-sin(2.0 * PI * k / n_fft));
    // lower edge 0, upper edge sr // 2 (vad_dataloader.py:109-115)
    if (mel_matrix(n_mels, n_bins, sample_rate, 0.0, (double)(sample_rate / 2), dense.data()) != SELD_OK) return SELD_ERR_INVALID;
    std::vector<int> mstart(n_mels, 0), mcnt(n_mels, 0), moff(n_mels, 0);
    for (int m = 0; m < n_mels; ++m) {      // a triangle's support is one contiguous run of bins
        int k0 = -1, k1 = -1;
        for (int k = 0; k < n_bins; ++k)
            if (dense[(size_t)k * n_mels + m] != 0.f) { if (k0 < 0) k0 = k; k1 = k; }
        moff[m] = (int)mw.size();
        if (k0 < 0) continue;
        mstart[m] = k0, mcnt[m] = k1 - k0 + 1;
        for (int k = k0; k <= k1; ++k) mw.push_back(dense[(size_t)k * n_mels + m]);
    }
    if (mw.empty()) mw.push_back(0.f);
    // the tables are allocated on `device`; the caller's current device is put back on every way out
    int prev = 0;
    if (hipGetDevice(&prev) != hipSuccess || hipSetDevice(device) != hipSuccess) return SELD_ERR_HIP;
    struct Restore { int d; ~Restore() { hipSetDevice(d); } } restore{prev};
    seld_vadfeat* f = new seld_vadfeat();
    f->device = device, f->sample_rate = sample_rate, f->n_fft = n_fft, f->n_mels = n_mels, f->n_melw = (int)mw.size();
    bool okk = true;
    okk &= hipMalloc(&f->win, n_fft * sizeof(float)) == hipSuccess;
    okk &= hipMalloc(&f->tw_half, twh.size() * sizeof(float2)) == hipSuccess;
    okk &= hipMalloc(&f->tw_full, twf.size() * sizeof(float2)) == hipSuccess;
    okk &= hipMalloc(&f->mel_start, n_mels * sizeof(int)) == hipSuccess;
    okk &= hipMalloc(&f->mel_cnt, n_mels * sizeof(int)) == hipSuccess;
    okk &= hipMalloc(&f->mel_off, n_mels * sizeof(int)) == hipSuccess;
    okk &= hipMalloc(&f->mel_w, mw.size() * sizeof(float)) == hipSuccess;
    if (!okk) { seld_vad_feat_destroy(f); return SELD_ERR_NOMEM; }
    okk &= hipMemcpy(f->win, win.data(), n_fft * sizeof(float), hipMemcpyHostToDevice) == hipSuccess;
    okk &= hipMemcpy(f->tw_half, twh.data(), twh.size() * sizeof(float2), hipMemcpyHostToDevice) == hipSuccess;
    okk &= hipMemcpy(f->tw_full, twf.data(), twf.size() * sizeof(float2), hipMemcpyHostToDevice) == hipSuccess;
    okk &= hipMemcpy(f->mel_start, mstart.data(), n_mels * sizeof(int), hipMemcpyHostToDevice) == hipSuccess;
    okk &= hipMemcpy(f->mel_cnt, mcnt.data(), n_mels * sizeof(int), hipMemcpyHostToDevice) == hipSuccess;
    okk &= hipMemcpy(f->mel_off, moff.data(), n_mels * sizeof(int), hipMemcpyHostToDevice) == hipSuccess;
    okk &= hipMemcpy(f->mel_w, mw.data(), mw.size() * sizeof(float), hipMemcpyHostToDevice) == hipSuccess;
    // above 64 KB of dynamic LDS (n_fft 2048) the kernel needs its limit raised: once, here
    const size_t smem = vf_smem(n_fft, n_mels, f->n_melw);
    const void* kern = n_fft == 512 ? reinterpret_cast<const void*>(vad_feat_kernel<8>)
                     : n_fft == 1024 ? reinterpret_cast<const void*>(vad_feat_kernel<9>) : reinterpret_cast<const void*>(vad_feat_kernel<10>);
    if (smem > 64 * 1024) okk &= hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) == hipSuccess;
    if (!okk) { seld_vad_feat_destroy(f); return SELD_ERR_HIP; }
    *out = f;
    return SELD_OK;
}

#define VAD_FEAT_CASE(LOGM_)                                                                                                              \
    case LOGM_: {                                                                                                                         \
        hipLaunchKernelGGL(vad_feat_kernel<LOGM_>, dim3(grid), dim3(64 * VF_WAVES), smem, st, wav, sample_starts, frame_starts, n_files,  \
                           total_samples, total_frames, f->n_mels, f->n_melw, f->win, f->tw_half, f->tw_full, f->mel_start, f->mel_cnt,   \
                           f->mel_off, f->mel_w, out);                                                                                    \
        break;                                                                                                                            \
    }

int seld_vad_feat_extract(seld_vadfeat* f, const float* wav, const int64_t* sample_starts, const int64_t* frame_starts, int n_files,
                          int64_t total_samples, int64_t total_frames, int logmel, int normalize, float* out, void* stream) {
    if (!f || !wav || !sample_starts || !frame_starts || !out || n_files < 1 || total_frames < 1 || total_samples < f->n_fft)
        return SELD_ERR_INVALID;
    if (total_frames > ((int64_t)1 << 40) / f->n_mels) return SELD_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const size_t smem = vf_smem(f->n_fft, f->n_mels, f->n_melw);
    // persistent waves, 1 024 workgroups at most (a grid cut to the resident workgroups measured the same)
    const int64_t want = (total_frames + VF_WAVES - 1) / VF_WAVES;
    const unsigned grid = (unsigned)(want < 1024 ? want : 1024);
    switch (logm_of(f->n_fft)) {
        VAD_FEAT_CASE(8)
        VAD_FEAT_CASE(9)
        VAD_FEAT_CASE(10)
        default: return SELD_ERR_UNSUPPORTED;
    }
    if (logmel || normalize)
        hipLaunchKernelGGL(vad_feat_post_kernel, dim3((unsigned)n_files), dim3(256), 0, st, out, frame_starts, total_frames, f->n_mels, logmel ? 1 : 0,
                           normalize ? 1 : 0);
    return ok();
}

int seld_vad_frame_labels(const float* labels, const int64_t* sample_starts, const int64_t* frame_starts, int n_files, int64_t total_samples,
                          int64_t total_frames, int n_fft, float* y, void* stream) {
    if (!labels || !sample_starts || !frame_starts || !y || n_files < 1 || total_frames < 1 || n_fft < 2 || (n_fft & 1) || total_samples < n_fft)
        return SELD_ERR_INVALID;
    if (total_frames > (int64_t)0x7fffffff * 4) return SELD_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(vad_frame_labels_kernel, dim3((unsigned)((total_frames + 3) / 4)), dim3(256), 0, (hipStream_t)stream, labels, sample_starts,
                       frame_starts, n_files, total_samples, total_frames, n_fft, y);
    return ok();
}

int seld_vad_gather(const float* feat, const float* y, const int64_t* pos, const int32_t* offs, int Wn, int B, int D, int64_t total_frames,
                    float* x_out, float* y_out, void* stream) {
    if (!feat || !y || !pos || !x_out || !y_out || B < 1 || D < 1 || total_frames < 1) return SELD_ERR_INVALID;
    WinTable tb;
    const int rc = win_table(offs, Wn, tb);
    if (rc != SELD_OK) return rc;
    if ((int64_t)B * Wn > (int64_t)0x7fffffff * 256 / D) return SELD_ERR_UNSUPPORTED;      // B Wn D elements, one thread each; no overflow on the way
    const int64_t total = (int64_t)B * Wn * D;
    hipLaunchKernelGGL(vad_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, feat, y, pos, total, D,
                       total_frames, x_out, y_out, tb);
    return ok();
}

int seld_vad_score_update(const float* pred, const float* y, int64_t n, const float* thresholds, int NT, int64_t* counts, void* stream) {
    if (!pred || !y || !thresholds || !counts || n < 1 || NT < 1) return SELD_ERR_INVALID;
    if (NT > SCORE_MAX_NT || n > ((int64_t)1 << 40)) return SELD_ERR_UNSUPPORTED;      // a workgroup's 32-bit buckets hold n / grid elements
    const int64_t want = (n + 255) / 256;
    hipLaunchKernelGGL(vad_score_kernel, dim3((unsigned)(want < 1024 ? want : 1024)), dim3(256), 0, (hipStream_t)stream, pred, y, n, thresholds, NT,
                       reinterpret_cast<unsigned long long*>(counts));
    return ok();
}

}  // extern "C"
