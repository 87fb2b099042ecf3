// mcs.hip — transforms.mcs_aug (transforms.py:202-291): the CGMM (complex-Gaussian mixture model) mask estimator, float64, in ONE launch.
// One workgroup owns one (b, f) column of x [B,T,F,C] for the whole call: initialisation, every EM round and the final product.
//   per-frame state   v_t (C floats) in LDS, the two phi and the two lambda (doubles) of up to MCS_K frames per thread in registers, across the
//                     rounds: x is read once and out is written once
//   time sums         per class C(C+1)/2 weighted products v_i v_j and one sum of lambda: formed per thread, reduced in the wave by a
//                     reduce-scatter over groups of 16 values (17 shuffles per group), then over the waves in wave order through LDS.  No
//                     atomic operation: the order is fixed, two calls give the same bits
//   small matrices    wave 0 takes class y, wave 1 class n.  Lane k holds column k of the symmetric C x C matrix in registers.  cond =
//                     |lambda|max / |lambda|min from cyclic Jacobi sweeps (the matrix is symmetric positive semi-definite: its singular values
//                     are its eigenvalues); the rotation's row half is local to a lane, its column half goes through v_readlane.  stab's
//                     tests need one eigen-solve: the eigenvalues of R + a I are those of R plus a.  Inverse and determinant by Gauss-Jordan
//                     on [A | I] without pivoting (A is positive definite after stab; the pivots are the squares of the Cholesky diagonal),
//                     lanes 0..C-1 holding A's columns and lanes C..2C-1 the identity's
#include "common.h"

#include <math.h>
#include <stdint.h>
#include "../../include/seld_hip.h"

#define MCS_MAX_C 10
#define MCS_K 6                 // frames per thread
#define MCS_MAX_THREADS 512
#define MCS_MAX_FRAMES (MCS_K * MCS_MAX_THREADS)
#define MCS_PITCH(C) ((C) | 1)      // floats per frame in LDS

namespace {

__device__ __forceinline__ double mcs_rl(double x, int lane) {      // x of lane `lane` (wave-uniform), through the scalar unit
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), lane), hi = __builtin_amdgcn_readlane(__double2hiint(x), lane);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double mcs_sdiv(double a, double y) { return a / fmax(y, 1e-8); }      // utils.safe_div

// index of (i, j), i <= j, in the row-major upper triangle of a C x C matrix
__device__ __forceinline__ int mcs_pair(int C, int i, int j) { return i * C - i * (i - 1) / 2 + (j - i); }

// 16 values per lane -> their 16 sums over the wave: lane L ends with the sum of value L >> 2 (every lane of a quad holds it).  Each step halves
// the values a lane keeps and adds the partner's half: 8 + 4 + 2 + 1 shuffles, then two plain steps.
__device__ __forceinline__ double mcs_reduce16(double (&r)[16], int lane) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int m = 32 >> s, half = 8 >> s;
        const bool up = lane & m;
#pragma unroll
        for (int i = 0; i < half; ++i) {
            const double send = up ? r[i] : r[i + half], keep = up ? r[i + half] : r[i];
            r[i] = keep + __shfl_xor(send, m);
        }
    }
    double s = r[0];
    s += __shfl_xor(s, 2);
    s += __shfl_xor(s, 1);
    return s;
}

template <int C>
__global__ __launch_bounds__(MCS_MAX_THREADS) void mcs_kernel(const float* x, float* out, double* __restrict__ lambda,
                                                              int32_t* __restrict__ stab_adds, int T, int F, int iteration, double theta) {
    constexpr int NP = C * (C + 1) / 2, NE = NP + 1, NG = (2 * NE + 15) / 16, K = MCS_K, CP = MCS_PITCH(C);
    extern __shared__ float vs[];            // [K * NT][CP]: v_t; the odd pitch keeps a wave's 64 frames of one channel on different banks
    __shared__ double red[MCS_MAX_THREADS / 64][NG * 16];
    __shared__ double S[NG * 16];            // NP products and the sum of lambda, class y and class n interleaved
    __shared__ double Minv[2][C * C];
    __shared__ double detA[2];
    const int tid = threadIdx.x, NT = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = NT >> 6;
    const int b = blockIdx.x / F, f = blockIdx.x - b * F;

    // frame t = k * NT + tid is this thread's for the whole call: nobody else reads its slot of vs, so no barrier guards it
    bool live[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int t = k * NT + tid;
        live[k] = t < T;
        const float* p = x + (((size_t)b * T + (live[k] ? t : 0)) * F + f) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) vs[t * CP + c] = live[k] ? p[c] : 0.f;
    }

    double lam[2][K], phi[2][K];
#pragma unroll
    for (int k = 0; k < K; ++k) lam[0][k] = lam[1][k] = phi[0][k] = phi[1][k] = 0.0;

    // S[2 * pair(i, j) + cl] = sum_t w[cl][t] v_t[i] v_t[j], S[2 * NP + cl] = sum_t lam[cl][t]; w = sdiv(lam, phi), or, for the
    // initialisation's R_y, 1 for class y
    auto time_sums = [&](bool first) {
        double w[2][K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            w[0][k] = first ? (live[k] ? 1.0 : 0.0) : mcs_sdiv(lam[0][k], phi[0][k]);
            w[1][k] = first ? 0.0 : mcs_sdiv(lam[1][k], phi[1][k]);
        }
        // a runtime loop over the groups, a running (i, j) over the pairs: unrolled, every group's products are formed before the first shuffle
        // and the registers run out
        int pi = 0, pj = 0;
#pragma unroll 1
        for (int g = 0; g < NG; ++g) {
            double r[16];
#pragma unroll
            for (int n = 0; n < 16; ++n) r[n] = 0.0;
#pragma unroll
            for (int n = 0; n < 16; n += 2) {      // the two classes of a pair side by side: one product serves both
                const int idx = g * 8 + (n >> 1);
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const double vv = (double)vs[(k * NT + tid) * CP + pi] * (double)vs[(k * NT + tid) * CP + pj];
                    r[n] += idx < NP ? w[0][k] * vv : (idx == NP ? lam[0][k] : 0.0);
                    r[n + 1] += idx < NP ? w[1][k] * vv : (idx == NP ? lam[1][k] : 0.0);
                }
                if (idx < NP - 1) {
                    if (++pj == C) { ++pi; pj = pi; }
                }
            }
            const double s = mcs_reduce16(r, lane);
            if ((lane & 3) == 0) red[wave][g * 16 + (lane >> 2)] = s;
        }
        __syncthreads();
        if (tid < NG * 16) {
            double s = 0.0;
            for (int q = 0; q < nw; ++q) s += red[q][tid];
            S[tid] = s;
        }
        __syncthreads();
    };

    // waves 0 and 1: R_cl from S, stab, then the inverse and determinant of the stabilised matrix.  Returns stab's number of additions.
    auto small_matrix = [&](int cl, bool first) -> int {
        const int kk = lane < C ? lane : 0;
        const double den = first ? (double)T : fmax(S[2 * NP + cl], 1e-8);
        auto load_R = [&](double (&a)[C]) {      // lane k < C: column k of R_cl; the other lanes zeros
#pragma unroll
            for (int i = 0; i < C; ++i) {
                const int lo = i < kk ? i : kk, hi = i < kk ? kk : i;
                double val = S[2 * mcs_pair(C, lo, hi) + cl] / den;
                if (first && cl == 1) val = i == kk ? 1.0 : 0.0;
                a[i] = lane < C ? val : 0.0;
            }
        };
        double col[C];
        load_R(col);
        // cyclic Jacobi: a sweep rotates every pair whose off-diagonal entry is above 1e-14 of the largest diagonal entry; done when none is
        for (int sweep = 0; sweep < 30; ++sweep) {
            double dmax = 0.0;
#pragma unroll
            for (int i = 0; i < C; ++i) dmax = fmax(dmax, fabs(mcs_rl(col[i], i)));
            const double tiny = 1e-14 * dmax;
            bool rotated = false;
#pragma unroll
            for (int p = 0; p < C - 1; ++p) {
#pragma unroll
                for (int q = p + 1; q < C; ++q) {
                    const double apq = mcs_rl(col[p], q);
                    if (!(fabs(apq) > tiny)) continue;
                    rotated = true;
                    const double app = mcs_rl(col[p], p), aqq = mcs_rl(col[q], q);
                    const double th = (aqq - app) / (2.0 * apq);
                    const double tt = copysign(1.0, th) / (fabs(th) + sqrt(th * th + 1.0));
                    const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
                    // A J: columns p and q
#pragma unroll
                    for (int i = 0; i < C; ++i) {
                        const double cp = mcs_rl(col[i], p), cq = mcs_rl(col[i], q);
                        col[i] = lane == p ? c * cp - s * cq : (lane == q ? s * cp + c * cq : col[i]);
                    }
                    // J^T (A J): rows p and q, local to every lane
                    const double xp = col[p], xq = col[q];
                    col[p] = c * xp - s * xq;
                    col[q] = s * xp + c * xq;
                    if (lane == p) col[q] = 0.0;
                    if (lane == q) col[p] = 0.0;
                }
            }
            if (!rotated) break;
        }
        double ev[C];
#pragma unroll
        for (int i = 0; i < C; ++i) ev[i] = mcs_rl(col[i], i);
        // stab (transforms.py:220-228), stopping at the first matrix that tests invertible: it no longer changes
        const double dd[6] = {1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1};
        double a0[C], add = 0.0;      // R again: the Jacobi copy is spent
        asm volatile("" ::: "memory");      // a second read of S, not 2 C registers kept through the sweeps
        load_R(a0);
        int adds = 0;
#pragma unroll
        for (int st = 0; st < 6; ++st) {
            double mx = 0.0, mn = INFINITY;
#pragma unroll
            for (int i = 0; i < C; ++i) {
                const double e = fabs(ev[i] + add);
                mx = fmax(mx, e);
                mn = fmin(mn, e);
            }
            const double cond = mx / mn;      // 0/0 (a zero matrix) is NaN: not invertible, like the infinite ratio the reference puts there
            if (cond < 1e6) break;            // false for NaN and for +inf
            add += dd[st];
#pragma unroll
            for (int i = 0; i < C; ++i)
                if (i == lane) a0[i] += dd[st];
            ++adds;
        }
        // Gauss-Jordan on [A | I]: lanes 0..C-1 hold A's columns, lanes C..2C-1 the identity's; a row operation is local to a lane
#pragma unroll
        for (int i = 0; i < C; ++i)
            if (lane >= C) a0[i] = lane - C == i ? 1.0 : 0.0;
        double det = 1.0;
#pragma unroll
        for (int k = 0; k < C; ++k) {
            const double piv = mcs_rl(a0[k], k);
            det *= piv;
            a0[k] *= 1.0 / piv;
            double fk[C];
#pragma unroll
            for (int i = 0; i < C; ++i) fk[i] = mcs_rl(a0[i], k);
#pragma unroll
            for (int i = 0; i < C; ++i)
                if (i != k) a0[i] -= fk[i] * a0[k];
        }
        if (lane >= C && lane < 2 * C) {
#pragma unroll
            for (int i = 0; i < C; ++i) Minv[cl][i * C + (lane - C)] = a0[i];
        }
        if (lane == 0) detA[cl] = det;
        return adds;
    };

    // q[cl] = v^T A_cl^-1 v of frame k: a runtime loop over the rows of the inverse, for the registers' sake as above
    auto quads = [&](int k, double (&q)[2]) {
        double vd[C];
#pragma unroll
        for (int c = 0; c < C; ++c) vd[c] = (double)vs[(k * NT + tid) * CP + c];
#pragma unroll
        for (int cl = 0; cl < 2; ++cl) {
            q[cl] = 0.0;
#pragma unroll 1
            for (int i = 0; i < C; ++i) {
                double s = 0.0;
#pragma unroll
                for (int j = 0; j < C; ++j) s += Minv[cl][i * C + j] * vd[j];
                q[cl] += (double)vs[(k * NT + tid) * CP + i] * s;
            }
        }
    };

    // The frame loop is a runtime loop, so that the compiler works on one frame at a time (unrolled, it interleaves the frames and runs out of
    // registers).  phi and lam stay in registers: a pass works on element 0 and rotates the arrays, K passes put them back in place.
    auto rotate = [&](double (&a)[2][K]) {
#pragma unroll
        for (int cl = 0; cl < 2; ++cl) {
            const double a0 = a[cl][0];
#pragma unroll
            for (int k = 0; k + 1 < K; ++k) a[cl][k] = a[cl][k + 1];
            a[cl][K - 1] = a0;
        }
    };
    int adds = 0;
    int32_t* sa = stab_adds ? stab_adds + ((size_t)blockIdx.x * 2 + (wave & 1)) * (iteration + 1) : nullptr;
    for (int r = 0; r <= iteration; ++r) {      // r = 0: the initialisation
        const bool first = r == 0;
        if (r != 1) {      // round 1 tests the matrices of the initialisation again: same additions, same inverse
            time_sums(first);      // its barriers also put every read of Minv and detA behind the writes below
            if (wave < 2) adds = small_matrix(wave, first);
            __syncthreads();
        }
        if (wave < 2 && sa && lane == 0) sa[r] = adds;
        const double det_y = detA[0], det_n = detA[1];
#pragma unroll 1
        for (int k = 0; k < K; ++k) {
            if (k * NT >= T) {      // no thread has a frame here: lam stays 0
                rotate(phi);
                rotate(lam);
                continue;
            }
            double p[2], q[2];
            quads(k, q);
            if (!first) {
#pragma unroll
                for (int cl = 0; cl < 2; ++cl) {
                    const double kq = mcs_sdiv(q[cl], phi[cl][0]);
                    double pw = 1.0;
#pragma unroll
                    for (int c = 0; c < C; ++c) pw *= phi[cl][0];
                    const double d = M_PI * (pw * (cl ? det_n : det_y));      // det(phi A) = phi^C det A
                    p[cl] = mcs_sdiv(exp(-kq), d) + theta;
                }
                const double ps = p[1] + p[0];
                const bool alive = k * NT + tid < T;
                lam[0][0] = alive ? mcs_sdiv(p[0], ps) : 0.0;
                lam[1][0] = alive ? mcs_sdiv(p[1], ps) : 0.0;
            }
            phi[0][0] = q[0] / C;
            phi[1][0] = q[1] / C;
            rotate(phi);
            rotate(lam);
        }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if (!live[k]) continue;
        const size_t row = ((size_t)b * T + (k * NT + tid)) * F + f;
        const float m = (float)lam[1][k];
        float* o = out + row * C;
#pragma unroll
        for (int c = 0; c < C; ++c) o[c] = vs[(k * NT + tid) * CP + c] * m;
        if (lambda) lambda[row] = lam[1][k];
    }
}

template <int C>
void mcs_launch(const float* x, float* out, double* lambda, int32_t* stab_adds, int B, int T, int F, int iteration, double theta, hipStream_t st) {
    int nt = ((T + MCS_K - 1) / MCS_K + 63) / 64 * 64;      // two waves at least: one per class in the small-matrix section
    nt = nt < 128 ? 128 : nt;
    const size_t smem = (size_t)MCS_PITCH(C) * MCS_K * nt * sizeof(float);
    if (smem > 48 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(mcs_kernel<C>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) != hipSuccess)
        return;      // the launch below then fails and reports it
    hipLaunchKernelGGL((mcs_kernel<C>), dim3((unsigned)(B * F)), dim3(nt), smem, st, x, out, lambda, stab_adds, T, F, iteration, theta);
}

}  // namespace

extern "C" {

int seld_aug_mcs_max_frames(int C) { return C >= 1 && C <= MCS_MAX_C ? MCS_MAX_FRAMES : 0; }

int seld_aug_mcs(const float* x, float* out, double* lambda, int32_t* stab_adds, int B, int T, int F, int C, int iteration, double theta,
                 void* stream) {
    if (!x || !out || B < 1 || T < 1 || F < 1 || iteration < 1) return SELD_ERR_INVALID;
    if (!(theta >= 0.0) || !isfinite(theta)) return SELD_ERR_INVALID;
    if (C < 1 || C > MCS_MAX_C || T > MCS_MAX_FRAMES || (int64_t)B * F > 0x7fffffff) return SELD_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    switch (C) {
#define MCS_CASE(n) case n: mcs_launch<n>(x, out, lambda, stab_adds, B, T, F, iteration, theta, st); break;
        MCS_CASE(1) MCS_CASE(2) MCS_CASE(3) MCS_CASE(4) MCS_CASE(5) MCS_CASE(6) MCS_CASE(7) MCS_CASE(8) MCS_CASE(9) MCS_CASE(10)
#undef MCS_CASE
    }
    return hipGetLastError() == hipSuccess ? SELD_OK : SELD_ERR_HIP;
}

}  // extern "C"
