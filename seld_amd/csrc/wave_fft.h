// wave_fft.h — the one-wave radix-4 Stockham transform of features.hip's wave-per-frame kernel, shared with vad_feat.hip.  One WAVE owns a
// transform end to end, so nothing in it needs a workgroup barrier: a wave's LDS instructions execute in order, which makes every exchange
// between its lanes a plain write followed by a read.  oracle/features_oracle.py::stockham_fft_radix4 is the index model: log4(N) passes
// (and a final radix-2 pass when log2(N) is odd), each lane holds N/256 butterflies in registers, a pass reads ALL its inputs and then
// writes IN PLACE (one N-point buffer per transform).  Lengths: N = 256, 512, 1024.  `tw` is exp(-2 pi i t / N) for t in [0, N/2).
#pragma once
#include <hip/hip_runtime.h>

namespace {

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

template <int LOGN>
struct WF {
    static constexpr int N = 1 << LOGN;
    static constexpr int NB4 = N / 256;           // radix-4 butterflies per lane and pass
    static constexpr int NB2 = N / 128;           // radix-2 butterflies per lane (final pass when LOGN is odd)
    static constexpr int P4 = LOGN / 2;
    static constexpr bool HAS2 = (LOGN & 1) != 0;
    static constexpr int NB = N / 2 + 1;
    static constexpr int NBP = NB + 3;            // row stride of the per-bin value planes
    static constexpr int NBI = (NB + 63) / 64;    // bins per lane
};

__device__ __forceinline__ float2 tw_at(const float2* tw, int t, int halfN) {   // exp(-2 pi i t / N), t in [0, N)
    float2 w = tw[t & (halfN - 1)];
    if (t & halfN) { w.x = -w.x; w.y = -w.y; }
    return w;
}
// lanes of one wave exchange data through LDS with no barrier: LDS executes a wave's instructions in order; this only stops
// the COMPILER from moving a lane's later read above its earlier write (to it they are unrelated addresses)
#define WAVE_LDS_FENCE() asm volatile("" ::: "memory")

// radix-4 passes 1 .. P4-1 and the optional final radix-2 pass of NF transforms, in place on buf[f]; `v` holds pass 0's
// inputs (element lane + 64 b + q N/4) when FROM_REGS, otherwise pass 0 reads them from buf[f] too
template <int LOGN, int NF, bool FROM_REGS>
__device__ __forceinline__ void wave_fft(float2 (&v)[NF][WF<LOGN>::NB4][4], float2* const (&buf)[NF], const float2* tw, int lane) {
    using G = WF<LOGN>;
    constexpr int N = G::N, NB4 = G::NB4, Q = N / 4;
#pragma unroll
    for (int s = 0; s < G::P4; ++s) {
        const int L = 1 << (2 * s);
        if (s > 0 || !FROM_REGS) {
#pragma unroll
            for (int f = 0; f < NF; ++f)
#pragma unroll
                for (int b = 0; b < NB4; ++b)
#pragma unroll
                    for (int q = 0; q < 4; ++q) v[f][b][q] = buf[f][lane + 64 * b + q * Q];
        }
#pragma unroll
        for (int b = 0; b < NB4; ++b) {
            const int j = lane + 64 * b, k = j & (L - 1);
            float2 w1 = make_float2(1.f, 0.f), w2 = w1, w3 = w1;
            if (s > 0) {
                const int ts = k * (N / (4 * L));
                w1 = tw_at(tw, ts, N / 2); w2 = tw_at(tw, 2 * ts, N / 2); w3 = tw_at(tw, 3 * ts, N / 2);
            }
#pragma unroll
            for (int f = 0; f < NF; ++f) {
                const float2 a0 = v[f][b][0];
                const float2 a1 = s > 0 ? cmul(w1, v[f][b][1]) : v[f][b][1];
                const float2 a2 = s > 0 ? cmul(w2, v[f][b][2]) : v[f][b][2];
                const float2 a3 = s > 0 ? cmul(w3, v[f][b][3]) : v[f][b][3];
                const float2 t0 = make_float2(a0.x + a2.x, a0.y + a2.y), t1 = make_float2(a0.x - a2.x, a0.y - a2.y);
                const float2 t2 = make_float2(a1.x + a3.x, a1.y + a3.y);
                const float2 t3 = make_float2(a1.y - a3.y, a3.x - a1.x);          // -i (a1 - a3)
                v[f][b][0] = make_float2(t0.x + t2.x, t0.y + t2.y);
                v[f][b][1] = make_float2(t1.x + t3.x, t1.y + t3.y);
                v[f][b][2] = make_float2(t0.x - t2.x, t0.y - t2.y);
                v[f][b][3] = make_float2(t1.x - t3.x, t1.y - t3.y);
            }
        }
        WAVE_LDS_FENCE();        // every input of the pass is in registers before the first in-place write
#pragma unroll
        for (int f = 0; f < NF; ++f)
#pragma unroll
            for (int b = 0; b < NB4; ++b) {
                const int j = lane + 64 * b, k = j & (L - 1), o = 4 * (j - k) + k;
#pragma unroll
                for (int p = 0; p < 4; ++p) buf[f][o + p * L] = v[f][b][p];
            }
        WAVE_LDS_FENCE();
    }
    if (G::HAS2) {               // L = N/2: k = j, twiddle tw[j]
        constexpr int NB2 = G::NB2;
        float2 u[NF][NB2], x[NF][NB2];
#pragma unroll
        for (int f = 0; f < NF; ++f)
#pragma unroll
            for (int b = 0; b < NB2; ++b) {
                const int j = lane + 64 * b;
                u[f][b] = buf[f][j];
                x[f][b] = cmul(tw[j], buf[f][j + N / 2]);
            }
        WAVE_LDS_FENCE();
#pragma unroll
        for (int f = 0; f < NF; ++f)
#pragma unroll
            for (int b = 0; b < NB2; ++b) {
                const int j = lane + 64 * b;
                buf[f][j] = make_float2(u[f][b].x + x[f][b].x, u[f][b].y + x[f][b].y);
                buf[f][j + N / 2] = make_float2(u[f][b].x - x[f][b].x, u[f][b].y - x[f][b].y);
            }
        WAVE_LDS_FENCE();
    }
}

}  // namespace
