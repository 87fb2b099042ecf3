// gru_w.hip — the GRU recurrence and its BPTT for ANY width u = 1..256 (seld_rnn_gruw_fwd / _bwd / _plan), exact fp32, Keras reset_after=True
// with gate order z | r | h: the equations of gru.hip:12-14 and the BPTT of gru.hip:228-232.  gru.hip's kernels are built around 128 units (U in
// the registers of one 512-thread workgroup, float4 staging of 16-byte aligned rows); these take the width at run time and assume nothing about
// alignment: every global access is ONE dword, so rows of u % 4 != 0 floats need no special case.
//
// A workgroup (256 threads) owns T clips of ONE direction for the whole sequence; workgroups never talk to each other, nothing is atomic, and
// every sum runs in a fixed order that depends neither on the batch nor on the clip's place in the tile.
//   width class UP = 8, 16, 32, 64, 128, 256 (the power of two >= u; lanes j >= u repeat unit u - 1 and store nothing)
//   thread (cg = tid / UP, j = tid % UP) carries unit j of the CPT clips cg * CPT .. + CPT - 1:  T = (256 / UP) * CPT
//   form 0 (u <= 64):  U (3 u^2 floats <= 48 KiB) is copied to LDS once;  CPT = 2:  T = 64, 32, 16, 8
//   form 1 (u  > 64):  U does not fit beside anything else (3 u^2 = 49 152 floats at 128, 196 608 at 256), so it is re-read every step
//                      through L1 / L2 with coalesced dword loads and each value read serves the thread's CPT clips;  T = 4
// Forward step: gh = h U is one fmaf chain over k per (clip, gate) — h comes from a double-buffered LDS vector [k][clip] (a broadcast read of
// CPT adjacent floats), U[k][g u + j] from LDS or memory with the lanes along j.  One LDS-only barrier per step.  Form 1 issues the loads
// of GW_KB rows of U together, pinned ahead of their FMAs: left to the compiler they sat beside their uses, three in flight, and a step was
// a chain of L2 round trips (15.9 us per step at 128 units, 5.1 with the batches: profiles/gru_width.json).
// Backward step: (A) thread (cg, j) forms the gate gradients of its clips, stores dgx / dgh and leaves dgh in LDS; (B) the product dgh U^T.
//   form 0: U's LDS copy has an ODD row stride, so thread (cg, j) walks ROW j of U conflict-free against dgh[column][clip] (double buffered):
//           one fmaf chain per clip, the carry never leaves the thread's registers, one barrier per step.
//   form 1: a thread-per-unit walk of U^T in memory would touch 64 cache lines per load, so the product runs ROW PER WAVE: a wave reads
//           rows of U with its lanes along the 3u columns (coalesced, RB rows in flight), multiplies by the clips' dgh held in registers and
//           sums over the wave with DPP adds and four v_readlane; lane 0 leaves the sum in LDS for the unit's thread.  Two barriers per step.
// Global operands stay off the step's dependent chain: each thread loads its own gx (forward) / dh, saved, h_prev (backward) values GW_PF /
// GW_PB steps ahead into a register ring (the loop is unrolled by the ring depth), so the wait in front of a step is for loads issued that
// many steps earlier.  These depths are what seld_rnn_gruw_plan reports as the staging chunks.
#include "common.h"

#define GW_NT 256
#define GW_PF 4      // forward: steps a thread's gx values are loaded ahead
#define GW_PB 2      // backward
#define GW_KB 16     // forward, form 1: rows of U a lane has in flight (divides the width classes 128 and 256)
#define GW_FORMS 2

static inline int gw_up(int u) { int up = 8; while (up < u) up *= 2; return up; }
static inline int gw_cpt(int up) { return up == 256 ? 4 : 2; }

__device__ __forceinline__ float gw_sigmoid(float x) { return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(x * -L2E)); }
__device__ __forceinline__ float gw_tanh(float x) { return fmaf(__builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(x * (2.f * L2E))), -2.f, 1.f); }

// sum over the 64 lanes in a fixed order, the same value in every lane
__device__ __forceinline__ float gw_wave_sum(float v) {
    v += dpp<0xB1 /*quad_perm [1,0,3,2]*/>(v);
    v += dpp<0x4E /*quad_perm [2,3,0,1]*/>(v);
    v += dpp<0x128 /*row_ror:8*/>(v);
    v += dpp<0x124 /*row_ror:4*/>(v);      // every lane: the sum of its row of 16
    const int vi = __float_as_int(v);
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(vi, 0)), r1 = __int_as_float(__builtin_amdgcn_readlane(vi, 16)),
                r2 = __int_as_float(__builtin_amdgcn_readlane(vi, 32)), r3 = __int_as_float(__builtin_amdgcn_readlane(vi, 48));
    return (r0 + r1) + (r2 + r3);
}

// ndir = 2: blockIdx = 2 * clip tile + direction;  ndir = 1: blockIdx = clip tile, the *_b arguments are NULL
template <int UP, int CPT, bool ULDS>
__global__ __launch_bounds__(GW_NT) void gruw_fwd_kernel(const float* __restrict__ gx_f, const float* __restrict__ gx_b, const float* __restrict__ U_f,
        const float* __restrict__ U_b, const float* __restrict__ brec_f, const float* __restrict__ brec_b, float* __restrict__ h_f,
        float* __restrict__ h_b, float* __restrict__ sv_f, float* __restrict__ sv_b, int B, int S, int u, int ndir) {
    constexpr int T = (GW_NT / UP) * CPT;
    const int dir = ndir == 2 ? (int)(blockIdx.x & 1) : 0;
    const int b0 = (ndir == 2 ? (int)(blockIdx.x >> 1) : (int)blockIdx.x) * T;
    const float* gx = dir ? gx_b : gx_f;
    const float* U = dir ? U_b : U_f;
    const float* brec = dir ? brec_b : brec_f;
    float* H = dir ? h_b : h_f;
    float* sv = dir ? sv_b : sv_f;      // NULL at inference: a uniform branch around the stores, the arithmetic of h is the same code
    const int tid = threadIdx.x, j = tid % UP, cg = tid / UP;
    const bool jok = j < u;
    const int jc = jok ? j : u - 1, u3 = 3 * u;
    __shared__ __attribute__((aligned(16))) float hl[2][UP * T];      // h[k][clip], double buffered
    __shared__ float Ul[ULDS ? 3 * UP * UP : 1];
    if constexpr (ULDS)
        for (int i = tid; i < u * u3; i += GW_NT) Ul[i] = U[i];
    for (int i = tid; i < 2 * UP * T; i += GW_NT) (&hl[0][0])[i] = 0.f;
    const float bz = brec[jc], br = brec[u + jc], bh = brec[2 * u + jc];
    bool bok[CPT];
    size_t rb[CPT];      // first row (clip * S) of the thread's clips; a clip past the batch reads clip B - 1 and stores nothing
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
        const int b = b0 + cg * CPT + i;
        bok[i] = b < B;
        rb[i] = (size_t)(bok[i] ? b : B - 1) * S;
    }
    float rz[GW_PF][CPT], rr[GW_PF][CPT], rh[GW_PF][CPT];      // the ring: gx of steps s .. s + GW_PF - 1
    auto load = [&](int p, int s) {
        const int t = dir ? S - 1 - s : s;
#pragma unroll
        for (int i = 0; i < CPT; ++i) {
            const float* g = gx + (rb[i] + t) * u3 + jc;
            rz[p][i] = g[0]; rr[p][i] = g[u]; rh[p][i] = g[2 * u];
        }
    };
#pragma unroll
    for (int p = 0; p < GW_PF; ++p)
        if (p < S) load(p, p);
    float hown[CPT];
#pragma unroll
    for (int i = 0; i < CPT; ++i) hown[i] = 0.f;
    __syncthreads();
    for (int s0 = 0; s0 < S; s0 += GW_PF) {
#pragma unroll
        for (int p = 0; p < GW_PF; ++p) {
            const int s = s0 + p;
            if (s < S) {      // uniform
                const int t = dir ? S - 1 - s : s, cur = s & 1;
                float xz[CPT], xr[CPT], xh[CPT];
#pragma unroll
                for (int i = 0; i < CPT; ++i) { xz[i] = rz[p][i] + bz; xr[i] = rr[p][i] + br; xh[i] = rh[p][i]; }
                if (s + GW_PF < S) load(p, s + GW_PF);
                float az[CPT], ar[CPT], ah[CPT];
#pragma unroll
                for (int i = 0; i < CPT; ++i) az[i] = ar[i] = ah[i] = 0.f;
                const float* hp = &hl[cur][cg * CPT];
                if constexpr (ULDS) {
#pragma unroll 4
                    for (int k = 0; k < u; ++k) {
                        const float uz = Ul[k * u3 + jc], ur = Ul[k * u3 + u + jc], uh = Ul[k * u3 + 2 * u + jc];
#pragma unroll
                        for (int i = 0; i < CPT; ++i) {
                            const float hv = hp[k * T + i];
                            az[i] = fmaf(hv, uz, az[i]); ar[i] = fmaf(hv, ur, ar[i]); ah[i] = fmaf(hv, uh, ah[i]);
                        }
                    }
                } else {
                    // GW_KB rows of U (3 GW_KB loads per lane) are in flight together, pinned ahead of their FMAs: issued beside their uses
                    // (the compiler's own order) a step was a chain of u / 1 L2 round trips.  Rows past u (the last batch; GW_KB divides
                    // UP) repeat row u - 1 and meet the zeros that lanes j >= u keep in h's rows u .. UP - 1
                    for (int k0 = 0; k0 < u; k0 += GW_KB) {
                        float uz[GW_KB], ur[GW_KB], uh[GW_KB];
#pragma unroll
                        for (int kk = 0; kk < GW_KB; ++kk) {
                            const float* up = U + min(k0 + kk, u - 1) * u3 + jc;
                            uz[kk] = up[0]; ur[kk] = up[u]; uh[kk] = up[2 * u];
                        }
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int kk = 0; kk < GW_KB; ++kk)
#pragma unroll
                            for (int i = 0; i < CPT; ++i) {
                                const float hv = hp[(k0 + kk) * T + i];
                                az[i] = fmaf(hv, uz[kk], az[i]); ar[i] = fmaf(hv, ur[kk], ar[i]); ah[i] = fmaf(hv, uh[kk], ah[i]);
                            }
                    }
                }
#pragma unroll
                for (int i = 0; i < CPT; ++i) {
                    const float z = gw_sigmoid(xz[i] + az[i]), r = gw_sigmoid(xr[i] + ar[i]);
                    const float ghh = ah[i] + bh;
                    const float hh = gw_tanh(fmaf(r, ghh, xh[i]));
                    const float hn = fmaf(z, hown[i] - hh, hh);      // z h + (1 - z) hh
                    hown[i] = hn;
                    hl[cur ^ 1][j * T + cg * CPT + i] = jok ? hn : 0.f;
                    if (jok && bok[i]) {
                        const size_t row = rb[i] + t;
                        H[row * u + j] = hn;
                        if (sv) {
                            float* d = sv + (row * u + j) * 4;      // saved gates [t][unit][z r hh gh]
                            d[0] = z; d[1] = r; d[2] = hh; d[3] = ghh;
                        }
                    }
                }
                lds_barrier();      // LDS only: the stores above and the ring's loads stay in flight
            }
        }
    }
}

// dO_*: the two directions' output gradients, used as given
template <int UP, int CPT, bool ULDS>
__global__ __launch_bounds__(GW_NT) void gruw_bwd_kernel(const float* __restrict__ dO_f, const float* __restrict__ dO_b, const float* __restrict__ h_f,
        const float* __restrict__ h_b, const float* __restrict__ sv_f, const float* __restrict__ sv_b, const float* __restrict__ U_f,
        const float* __restrict__ U_b, float* __restrict__ dgx_f, float* __restrict__ dgx_b, float* __restrict__ dgh_f, float* __restrict__ dgh_b,
        int B, int S, int u, int ndir) {
    constexpr int T = (GW_NT / UP) * CPT;
    constexpr int NCH = (3 * UP + 63) / 64, LD = NCH * 64;      // a lane of phase B owns columns lane + 64 i
    const int dir = ndir == 2 ? (int)(blockIdx.x & 1) : 0;
    const int b0 = (ndir == 2 ? (int)(blockIdx.x >> 1) : (int)blockIdx.x) * T;
    const float* dO = dir ? dO_b : dO_f;
    const float* H = dir ? h_b : h_f;
    const float* sv = dir ? sv_b : sv_f;
    const float* U = dir ? U_b : U_f;
    float* dgx = dir ? dgx_b : dgx_f;
    float* dgh = dir ? dgh_b : dgh_f;
    const int tid = threadIdx.x, j = tid % UP, cg = tid / UP, lane = tid & 63, wave = tid >> 6;
    const bool jok = j < u;
    const int jc = jok ? j : u - 1, u3 = 3 * u;
    // form 1: gl = dgh[clip][column] (columns >= 3u stay 0), cm = (dgh U^T)[clip][unit] of the step before.
    // form 0: gl = dgh[buffer][column][clip], double buffered (one barrier per step); U's rows at the ODD stride ldu, so that the lanes of a
    // wave, which read one column of 64 different rows, fall into 64 different banks; the product stays in the thread's registers (no cm)
    constexpr int GLN = ULDS ? 2 * 3 * UP * T : T * LD;
    __shared__ __attribute__((aligned(16))) float gl[GLN];
    __shared__ float cm[ULDS ? 1 : T * UP];
    __shared__ float Ul[ULDS ? UP * (3 * UP + 1) : 1];
    const int ldu = u3 | 1;
    if constexpr (ULDS)
        for (int i = tid; i < u * u3; i += GW_NT) Ul[(i / u3) * ldu + i % u3] = U[i];
    for (int i = tid; i < GLN; i += GW_NT) gl[i] = 0.f;
    if constexpr (!ULDS)
        for (int i = tid; i < T * UP; i += GW_NT) cm[i] = 0.f;
    bool bok[CPT];
    size_t rb[CPT];
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
        const int b = b0 + cg * CPT + i;
        bok[i] = b < B;
        rb[i] = (size_t)(bok[i] ? b : B - 1) * S;
    }
    // the forward consumed t = 0 .. S-1 (dir 0) / S-1 .. 0 (dir 1); BPTT step s is t = S-1-s (dir 0) / s (dir 1), h_prev(t) = H[t-1] / H[t+1]
    float q_do[GW_PB][CPT], q_z[GW_PB][CPT], q_r[GW_PB][CPT], q_hh[GW_PB][CPT], q_gh[GW_PB][CPT], q_hp[GW_PB][CPT];
    auto load = [&](int p, int s) {
        const int t = dir ? s : S - 1 - s, tp = dir ? t + 1 : t - 1;
        const bool pok = tp >= 0 && tp < S;
#pragma unroll
        for (int i = 0; i < CPT; ++i) {
            const size_t e = (rb[i] + t) * u + jc;
            q_do[p][i] = dO[e];
            const float* g = sv + e * 4;
            q_z[p][i] = g[0]; q_r[p][i] = g[1]; q_hh[p][i] = g[2]; q_gh[p][i] = g[3];
            const float hv = H[(rb[i] + (pok ? tp : t)) * u + jc];      // always in bounds
            q_hp[p][i] = pok ? hv : 0.f;
        }
    };
#pragma unroll
    for (int p = 0; p < GW_PB; ++p)
        if (p < S) load(p, p);
    float zdh[CPT];      // form 1: dh z of the step before;  form 0: the whole carry dh z + dgh U^T
#pragma unroll
    for (int i = 0; i < CPT; ++i) zdh[i] = 0.f;
    __syncthreads();
    for (int s0 = 0; s0 < S; s0 += GW_PB) {
#pragma unroll
        for (int p = 0; p < GW_PB; ++p) {
            const int s = s0 + p;
            if (s < S) {      // uniform
                const int t = dir ? s : S - 1 - s;
                float c_do[CPT], c_z[CPT], c_r[CPT], c_hh[CPT], c_gh[CPT], c_hp[CPT];
#pragma unroll
                for (int i = 0; i < CPT; ++i) {
                    c_do[i] = q_do[p][i]; c_z[i] = q_z[p][i]; c_r[i] = q_r[p][i]; c_hh[i] = q_hh[p][i]; c_gh[i] = q_gh[p][i]; c_hp[i] = q_hp[p][i];
                }
                if (s + GW_PB < S) load(p, s + GW_PB);
                // (A) gate gradients of unit j, clips cg * CPT + i
#pragma unroll
                for (int i = 0; i < CPT; ++i) {
                    const int cl = cg * CPT + i;
                    float dh;
                    if constexpr (ULDS) dh = c_do[i] + zdh[i];
                    else dh = c_do[i] + (zdh[i] + cm[cl * UP + j]);
                    const float omz = 1.f - c_z[i];
                    const float a_h = dh * omz * (1.f - c_hh[i] * c_hh[i]);
                    const float a_z = dh * (c_hp[i] - c_hh[i]) * c_z[i] * omz;
                    const float a_r = a_h * c_gh[i] * c_r[i] * (1.f - c_r[i]);
                    const float a_hr = a_h * c_r[i];
                    zdh[i] = dh * c_z[i];
                    if (jok) {
                        if constexpr (ULDS) {
                            float* gw = gl + (s & 1) * (3 * UP * T) + cl;
                            gw[j * T] = a_z; gw[(u + j) * T] = a_r; gw[(2 * u + j) * T] = a_hr;
                        } else {
                            gl[cl * LD + j] = a_z; gl[cl * LD + u + j] = a_r; gl[cl * LD + 2 * u + j] = a_hr;
                        }
                        if (bok[i]) {
                            const size_t o = (rb[i] + t) * u3 + j;
                            dgx[o] = a_z; dgx[o + u] = a_r; dgx[o + 2 * u] = a_h;
                            dgh[o] = a_z; dgh[o + u] = a_r; dgh[o + 2 * u] = a_hr;
                        }
                    }
                }
                lds_barrier();
                if constexpr (ULDS) {
                    // (B, form 0) the thread's own units: carry[clip] = dh z + sum over c of dgh[clip][c] U[j][c], one fmaf chain per clip
                    const float* gp = gl + (s & 1) * (3 * UP * T) + cg * CPT;
                    const float* up = Ul + jc * ldu;
                    float acc[CPT];
#pragma unroll
                    for (int i = 0; i < CPT; ++i) acc[i] = 0.f;
#pragma unroll 4
                    for (int c = 0; c < u3; ++c) {
                        const float uv = up[c];
#pragma unroll
                        for (int i = 0; i < CPT; ++i) acc[i] = fmaf(gp[c * T + i], uv, acc[i]);
                    }
#pragma unroll
                    for (int i = 0; i < CPT; ++i) zdh[i] += acc[i];
                    // no second barrier: the next step writes the other buffer, and this one is written again behind the next step's barrier
                } else {
                    // (B, form 1) cm[clip][jr] = sum over c of dgh[clip][c] U[jr][c]: wave w takes rows w, w + 4, ..., RB rows at a time so
                    // that the loads of RB rows are in flight together (a row at a time, the step was a chain of L2 round trips)
                    float g[T][NCH];
#pragma unroll
                    for (int cl = 0; cl < T; ++cl)
#pragma unroll
                        for (int i = 0; i < NCH; ++i) g[cl][i] = gl[cl * LD + lane + 64 * i];
                    constexpr int NW = GW_NT / 64;
                    constexpr int RB = UP == 128 ? 8 : 4;      // rows of U a wave has in flight: 48 loads per lane in both width classes
                    for (int j0 = wave; j0 < u; j0 += NW * RB) {
                        float ur[RB][NCH];
#pragma unroll
                        for (int rbk = 0; rbk < RB; ++rbk) {
                            const int jr = min(j0 + NW * rbk, u - 1);      // past the last row: that row again, not stored
#pragma unroll
                            for (int i = 0; i < NCH; ++i) {
                                const int c = lane + 64 * i;
                                ur[rbk][i] = U[jr * u3 + (c < u3 ? c : u3 - 1)];      // the row's last column again, times the 0 of gl's padding
                            }
                        }
                        __builtin_amdgcn_sched_barrier(0);      // the loads stay ahead of the first reduction
#pragma unroll
                        for (int rbk = 0; rbk < RB; ++rbk) {
                            const int jr = j0 + NW * rbk;
#pragma unroll
                            for (int cl = 0; cl < T; ++cl) {
                                float a = 0.f;
#pragma unroll
                                for (int i = 0; i < NCH; ++i) a = fmaf(g[cl][i], ur[rbk][i], a);
                                a = gw_wave_sum(a);
                                if (lane == 0 && jr < u) cm[cl * UP + jr] = a;
                            }
                        }
                    }
                    lds_barrier();
                }
            }
        }
    }
}

template <int UP, int CPT, bool ULDS>
static void gw_launch_fwd(hipStream_t st, int nblk, const float* gx_f, const float* gx_b, const float* U_f, const float* U_b, const float* brec_f,
                          const float* brec_b, float* h_f, float* h_b, float* sv_f, float* sv_b, int B, int S, int u, int ndir) {
    hipLaunchKernelGGL((gruw_fwd_kernel<UP, CPT, ULDS>), dim3(nblk), dim3(GW_NT), 0, st, gx_f, gx_b, U_f, U_b, brec_f, brec_b, h_f, h_b, sv_f, sv_b, B, S,
                       u, ndir);
}
template <int UP, int CPT, bool ULDS>
static void gw_launch_bwd(hipStream_t st, int nblk, const float* dh_f, const float* dh_b, const float* h_f, const float* h_b, const float* sv_f,
                          const float* sv_b, const float* U_f, const float* U_b, float* dgx_f, float* dgx_b, float* dgh_f, float* dgh_b, int B, int S,
                          int u, int ndir) {
    hipLaunchKernelGGL((gruw_bwd_kernel<UP, CPT, ULDS>), dim3(nblk), dim3(GW_NT), 0, st, dh_f, dh_b, h_f, h_b, sv_f, sv_b, U_f, U_b, dgx_f, dgx_b, dgh_f,
                       dgh_b, B, S, u, ndir);
}
// one line per width class: UP, CPT, U in LDS
#define GW_DISPATCH(up, CALL)                   \
    switch (up) {                               \
        case 8: CALL(8, 2, true); break;        \
        case 16: CALL(16, 2, true); break;      \
        case 32: CALL(32, 2, true); break;      \
        case 64: CALL(64, 2, true); break;      \
        case 128: CALL(128, 2, false); break;   \
        default: CALL(256, 4, false); break;    \
    }

/* The kernels index rows (clip * S + t) and elements in 64 bits; B, S and the step counter s + GW_PF are ints, the grid is 2 * ceil(B / T) blocks:
 * B and S up to 2^30, and B * S up to 2^40 rows so that rows * 4u floats * 4 bytes stays below 2^54. */
#define GW_MAX_DIM 0x3fffffff
#define GW_MAX_ROWS ((int64_t)1 << 40)

extern "C" {
int seld_rnn_gruw_plan(int units, int32_t out[4]) {
    if (units < 1 || units > 256) return SELD_ERR_UNSUPPORTED;
    if (!out) return SELD_ERR_INVALID;
    const int up = gw_up(units);
    out[0] = up <= 64 ? 0 : 1;
    out[1] = (GW_NT / up) * gw_cpt(up);
    out[2] = GW_PF;
    out[3] = GW_PB;
    return GW_FORMS;
}
int seld_rnn_gruw_fwd(const float* gx_f, const float* gx_b, const float* U_f, const float* U_b, const float* brec_f, const float* brec_b, float* h_f,
                      float* h_b, float* saved_f, float* saved_b, int B, int S, int units, void* stream) {
    if (units < 1 || units > 256) return SELD_ERR_UNSUPPORTED;
    if (!gx_f || !U_f || !brec_f || !h_f || B < 1 || S < 1) return SELD_ERR_INVALID;
    if (gx_b ? (!U_b || !brec_b || !h_b || (!saved_b) != (!saved_f)) : (U_b || brec_b || h_b || saved_b)) return SELD_ERR_INVALID;
    if (S > GW_MAX_DIM || B > GW_MAX_DIM || (int64_t)B * S > GW_MAX_ROWS) return SELD_ERR_UNSUPPORTED;
    const int up = gw_up(units), tile = (GW_NT / up) * gw_cpt(up), ndir = gx_b ? 2 : 1;
    const int nblk = ndir * ((B + tile - 1) / tile);
#define GW_F(UP, CPT, ULDS) \
    gw_launch_fwd<UP, CPT, ULDS>((hipStream_t)stream, nblk, gx_f, gx_b, U_f, U_b, brec_f, brec_b, h_f, h_b, saved_f, saved_b, B, S, units, ndir)
    GW_DISPATCH(up, GW_F)
#undef GW_F
    return ok();
}
int seld_rnn_gruw_bwd(const float* dh_f, const float* dh_b, const float* h_f, const float* h_b, const float* saved_f, const float* saved_b,
                      const float* U_f, const float* U_b, float* dgx_f, float* dgx_b, float* dgh_f, float* dgh_b, int B, int S, int units,
                      void* stream) {
    if (units < 1 || units > 256) return SELD_ERR_UNSUPPORTED;
    if (!dh_f || !h_f || !saved_f || !U_f || !dgx_f || !dgh_f || B < 1 || S < 1) return SELD_ERR_INVALID;
    if (dh_b ? (!h_b || !saved_b || !U_b || !dgx_b || !dgh_b) : (h_b || saved_b || U_b || dgx_b || dgh_b)) return SELD_ERR_INVALID;
    if (S > GW_MAX_DIM || B > GW_MAX_DIM || (int64_t)B * S > GW_MAX_ROWS) return SELD_ERR_UNSUPPORTED;
    const int up = gw_up(units), tile = (GW_NT / up) * gw_cpt(up), ndir = dh_b ? 2 : 1;
    const int nblk = ndir * ((B + tile - 1) / tile);
#define GW_B(UP, CPT, ULDS) \
    gw_launch_bwd<UP, CPT, ULDS>((hipStream_t)stream, nblk, dh_f, dh_b, h_f, h_b, saved_f, saved_b, U_f, U_b, dgx_f, dgx_b, dgh_f, dgh_b, B, S, units, ndir)
    GW_DISPATCH(up, GW_B)
#undef GW_B
    return ok();
}
}
