// lstm.hip — recurrence of LSTM(128, return_sequences=True), alone or as the two layers of a Bidirectional (reference modules.RNN_block,
// modules.py:322-347, rnn_type != 'GRU'), forward and BPTT, exact fp32.  Keras defaults: gate order i | f | c | o, ONE bias (added on the
// input side: it is part of gx), activation tanh, recurrent_activation sigmoid:
//   z = gx[t] + h U;  i = s(z_i)  f = s(z_f)  g = tanh(z_c)  o = s(z_o);  c' = f c + i g;  h' = o tanh(c');  h(-1) = c(-1) = 0
//
// The form is gru.hip's (read its header first): ONE 512-thread workgroup per (clip, direction), U [128,512] in registers for the whole
// sequence (128 fp32 per thread), h exchanged through a double-buffered padded LDS vector with ONE LDS-only barrier per step, global operands
// staged per chunk of steps (loads issued at the start of a chunk, committed to LDS at its end) so that no global load sits on a step's
// critical path.  No atomics and fixed summation orders: two runs give the same bits.
//
// forward: thread (j = tid >> 2, q = tid & 3) = unit j, quarter q of the reduction axis.  Accumulator a of a lane holds gate a ^ q, so the
// fold over the quad is three DPP adds and leaves the whole sum of gate q in lane q: each lane then runs ONE activation (lane 2 the tanh, as
// 2 s(2x) - 1: the same instruction stream with per-lane constants), four quad_perm moves hand i, f, g, o to all four lanes, and every lane
// of the quad carries the unit's cell state c in a register for the whole sequence.
// BPTT: gru_bwd_kernel's register blocking of the transposed mat-vec (512 -> 128: 4 outputs x 32 columns per lane, 8 ds_read_b128 per step),
// and its 16 lanes per 4 units map onto (unit, gate i | f | g | o) exactly: no idle role.
//
// DROP (Keras LSTM recurrent_dropout, reference modules.py:338-340; training only): the previous state is multiplied by a per-(clip, unit) mask
// rm = 0 | 1 / (1 - rate), constant over the sequence, ahead of the recurrent product — LSTMCell.call, implementation 2: z = gx[t] + (h rm) U.
// c is never masked and the emitted h is the unmasked one.  A workgroup serves ONE clip for the whole sequence, so the mask is folded into the
// register copy of U while it is loaded and the step loop is the undropped kernel's, instruction for instruction:
//   forward: (h rm) U = h (diag(rm) U): row k of U is scaled by rm[b][k];
//   BPTT:    the carry rm (dz U^T) = dz (diag(rm) U)^T: row j of U^T's operand, i.e. the lane's output j, is scaled by rm[b][j].
// A mask of ones multiplies by 1.0f: the bits of the undropped kernels.
#include "common.h"

namespace {

// f32x2, pk_fma, dpp<CTRL> and L2E: common.h, shared with gru.hip
// branch-free, saturating: exp2 -> inf gives rcp -> 0 (abs error ~1e-7, the form gru.hip's step uses)
__device__ __forceinline__ float tanh_(float x) { return fmaf(-2.f, __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(x * (2.f * L2E))), 1.f); }

#define LSTM_U 128
#define LSTM_G 512
#define LSTMF_CH 16    // forward: steps per staged chunk (32 KB of gx per buffer)
#define LSTMB_CH 8     // backward
#define LSTMB_ROW 896  // floats staged per backward step: dh | i f g o (per unit) | c | c_prev
#define LSTMB_GL 576   // padded gate-gradient vector: column c lives at 36 * (c / 32) + c % 32 (16 parts, conflict-free b128 reads)
#define LSTM_HL 144    // padded h vector: index k lives at k + 4 * (k >> 5) (the 4 quarters start in different bank groups)

// SAVE: c [S][128] and the activations [S][unit][i f g o] are stored for the backward pass; the arithmetic of h does not depend on it
template <bool SAVE, bool DROP = false>
__global__ __launch_bounds__(512) void lstm_fwd_kernel(const float* __restrict__ gx_f, const float* __restrict__ gx_b,
                                                       const float* __restrict__ U_f, const float* __restrict__ U_b,
                                                       float* __restrict__ h_f, float* __restrict__ h_b, float* __restrict__ c_f,
                                                       float* __restrict__ c_b, float* __restrict__ sv_f, float* __restrict__ sv_b, int S,
                                                       int ndir, const float* __restrict__ rm_f = nullptr,
                                                       const float* __restrict__ rm_b = nullptr) {
    const int b = ndir == 2 ? blockIdx.x >> 1 : blockIdx.x, dir = ndir == 2 ? blockIdx.x & 1 : 0;
    const float* gx = (dir ? gx_b : gx_f) + (size_t)b * S * LSTM_G;
    const float* U = dir ? U_b : U_f;
    float* H = (dir ? h_b : h_f) + (size_t)b * S * LSTM_U;
    float* Cs = nullptr;
    float* sv = nullptr;
    if constexpr (SAVE) {
        Cs = (dir ? c_b : c_f) + (size_t)b * S * LSTM_U;
        sv = (dir ? sv_b : sv_f) + (size_t)b * S * LSTM_G;
    }
    const int tid = threadIdx.x, j = tid >> 2, q = tid & 3;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* gxl = smem;                                // [2][LSTMF_CH][512]
    float* hl = smem + 2 * LSTMF_CH * LSTM_G;         // [2][LSTM_HL]
    f32x2 u[4][16];   // u[a][p] = (U[32q+2p][(a^q)*128+j], U[32q+2p+1][(a^q)*128+j])
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int p = 0; p < 16; ++p) {
            const int col = (a ^ q) * LSTM_U + j;
            u[a][p].x = U[(size_t)(32 * q + 2 * p) * LSTM_G + col];
            u[a][p].y = U[(size_t)(32 * q + 2 * p + 1) * LSTM_G + col];
            if constexpr (DROP) {      // diag(rm) U: rows 32q + 2p, + 1
                const float* rm = (dir ? rm_b : rm_f) + (size_t)b * LSTM_U;
                u[a][p].x *= rm[32 * q + 2 * p];
                u[a][p].y *= rm[32 * q + 2 * p + 1];
            }
        }
    // lane q finishes gate q: sigmoid(x) = rcp(1 + exp2(-log2e x)); lane 2: tanh(x) = 2 rcp(1 + exp2(-2 log2e x)) - 1
    const float nsc = q == 2 ? -2.f * L2E : -L2E, am = q == 2 ? 2.f : 1.f, aa = q == 2 ? -1.f : 0.f;
    const int g_off = q * LSTM_U + j;
    if (tid < 2 * LSTM_HL) hl[tid] = 0.f;
    float c_own = 0.f, pre_n = 0.f;
    const unsigned h_off = 4u * j, sv_off = 4u * tid;
    const int nchunks = (S + LSTMF_CH - 1) / LSTMF_CH;
    float4 stg0, stg1, stg2, stg3;      // named registers, not an array: see gru_fwd_kernel's staged chunk
    // chunk c = processing steps [c*CH, c*CH+n); its rows are contiguous in memory from row tlo
#define LSTMF_CHUNK_ROWS(c, n, tlo)                    \
    {                                                  \
        const int s0_ = (c) * LSTMF_CH;                \
        n = min(LSTMF_CH, S - s0_);                    \
        tlo = dir ? S - s0_ - n : s0_;                 \
    }
#define LSTMF_ISSUE(c)                                                                             \
    {                                                                                              \
        int n_, tlo_;                                                                              \
        LSTMF_CHUNK_ROWS(c, n_, tlo_)                                                              \
        const float4* src_ = reinterpret_cast<const float4*>(gx + (size_t)tlo_ * LSTM_G);          \
        const int lim_ = n_ * (LSTM_G / 4);                                                        \
        stg0 = src_[tid < lim_ ? tid : 0];               /* rows past the chunk are never read */  \
        stg1 = src_[tid + 512 < lim_ ? tid + 512 : 0];                                             \
        stg2 = src_[tid + 1024 < lim_ ? tid + 1024 : 0];                                           \
        stg3 = src_[tid + 1536 < lim_ ? tid + 1536 : 0];                                           \
    }
#define LSTMF_COMMIT(buf)                                                                \
    {                                                                                    \
        float4* d_ = reinterpret_cast<float4*>(gxl + (buf) * LSTMF_CH * LSTM_G);         \
        d_[tid] = stg0; d_[tid + 512] = stg1; d_[tid + 1024] = stg2; d_[tid + 1536] = stg3; \
    }
    LSTMF_ISSUE(0)
    LSTMF_COMMIT(0)
    __syncthreads();
    int step = 0;
    for (int c = 0; c < nchunks; ++c) {
        int n, tlo;
        LSTMF_CHUNK_ROWS(c, n, tlo)
        LSTMF_ISSUE(min(c + 1, nchunks - 1))      // unconditional: see gru_fwd_kernel's chunk loop
        const float* gb = gxl + (c & 1) * LSTMF_CH * LSTM_G;
        // the step's input term is read from the staged chunk a step AHEAD, so the reads queued behind the barrier are the eight of h alone
        auto load_gx = [&](int i) {
            const int row = dir ? n - 1 - i : i;
            pre_n = gb[row * LSTM_G + g_off] * nsc;
        };
        auto do_step = [&](int i, bool prefetch) {
            const int row = dir ? n - 1 - i : i;
            const int t = tlo + row;
            const float* hp = hl + (step & 1) * LSTM_HL + 36 * q;
            const float pre = pre_n;
            float4 hv[8];
#pragma unroll
            for (int k4 = 0; k4 < 8; ++k4) hv[k4] = *reinterpret_cast<const float4*>(hp + 4 * k4);
            f32x2 s2[4] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
#pragma unroll
            for (int k4 = 0; k4 < 8; ++k4) {
                const f32x2 h01 = {hv[k4].x, hv[k4].y}, h23 = {hv[k4].z, hv[k4].w};
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    s2[a] = pk_fma(h01, u[a][2 * k4], s2[a]);
                    s2[a] = pk_fma(h23, u[a][2 * k4 + 1], s2[a]);
                }
            }
            // accumulator a holds gate a ^ q: the xor-1 neighbour's slot 1 (3) is this lane's slot 0 (2), the xor-2 neighbour's slot 2 its slot 0
            const float a0 = (s2[0].x + s2[0].y) + dpp<0xB1 /*quad_perm [1,0,3,2]*/>(s2[1].x + s2[1].y);
            const float a2 = (s2[2].x + s2[2].y) + dpp<0xB1>(s2[3].x + s2[3].y);
            const float zq = a0 + dpp<0x4E /*quad_perm [2,3,0,1]*/>(a2);
            const float av = fmaf(am, __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(fmaf(zq, nsc, pre))), aa);
            const float gi = dpp<0x00>(av), gf = dpp<0x55>(av), gg = dpp<0xAA>(av), go = dpp<0xFF>(av);
            c_own = fmaf(gf, c_own, gi * gg);
            const float rc = __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(c_own * (2.f * L2E)));
            const float hn = fmaf(-2.f * go, rc, go);      // o tanh(c')
            // all four lanes of a quad hold the same hn and store it to the same word: the step body stays ONE basic block (gru_fwd_kernel's do_step)
            hl[((step + 1) & 1) * LSTM_HL + j + 4 * (j >> 5)] = hn;
            __builtin_amdgcn_sched_barrier(0);      // the exchange write leaves first; output stores and the next step's input term follow
            *reinterpret_cast<float*>(reinterpret_cast<char*>(H) + ((unsigned)t * (LSTM_U * 4u) + h_off)) = hn;
            if (prefetch) load_gx(i + 1);
            if constexpr (SAVE) {
                *reinterpret_cast<float*>(reinterpret_cast<char*>(Cs) + ((unsigned)t * (LSTM_U * 4u) + h_off)) = c_own;
                *reinterpret_cast<float*>(reinterpret_cast<char*>(sv) + ((unsigned)t * (LSTM_G * 4u) + sv_off)) = av;      // [t][unit][i f g o]
            }
            ++step;
        };
        load_gx(0);
        for (int i = 0; i < n - 1; ++i) {
            do_step(i, true);
            lds_barrier();   // LDS-only: __syncthreads() would also wait for this step's global stores
        }
        do_step(n - 1, false);
        LSTMF_COMMIT((c + 1) & 1)  // the only wait on the staged loads: one chunk after their issue
        lds_barrier();
    }
}

// BPTT (reverse of the forward processing order), dh[t] = the gradient w.r.t. this direction's output, carries dh_c (all lanes of a unit) and dc_c:
//   dh = dh[t] + dh_c;  dc = dh o (1 - tanh^2(c')) + dc_c;  dz_i = dc g i(1-i)  dz_f = dc c_prev f(1-f)  dz_c = dc i (1-g^2)  dz_o = dh tanh(c') o(1-o)
//   dc_c = dc f;  dh_c = dz U^T;  dgx[t] = dz
// Lane (grp = lane >> 4, cp = lane & 15) of wave w owns the outputs j0..j0+3 (j0 = 4 (4w + grp)) of the mat-vec over the 32 columns
// [32cp, 32cp+32), U^T's four rows in the order a ^ (cp & 3) (as gru_bwd_kernel), and the gate gradient of (unit j0 + (cp & 3), gate cp >> 2).
// Everything of a step except dh and dc is prepared by pre() for the NEXT step while this step's mat-vec runs: behind the carry sit one add, two
// fma and one multiply.
template <bool DROP = false>
__global__ __launch_bounds__(512) void lstm_bwd_kernel(const float* __restrict__ dh_f, const float* __restrict__ dh_b,
                                                       const float* __restrict__ c_f, const float* __restrict__ c_b,
                                                       const float* __restrict__ sv_f, const float* __restrict__ sv_b,
                                                       const float* __restrict__ U_f, const float* __restrict__ U_b,
                                                       float* __restrict__ dgx_f, float* __restrict__ dgx_b, int S, int ndir,
                                                       const float* __restrict__ rm_f = nullptr, const float* __restrict__ rm_b = nullptr) {
    const int b = ndir == 2 ? blockIdx.x >> 1 : blockIdx.x, dir = ndir == 2 ? blockIdx.x & 1 : 0;
    const float* dO = (dir ? dh_b : dh_f) + (size_t)b * S * LSTM_U;
    const float* Cs = (dir ? c_b : c_f) + (size_t)b * S * LSTM_U;
    const float* sv = (dir ? sv_b : sv_f) + (size_t)b * S * LSTM_G;
    const float* U = dir ? U_b : U_f;
    float* dgx = (dir ? dgx_b : dgx_f) + (size_t)b * S * LSTM_G;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cp = lane & 15;                       // column part of the mat-vec
    const int j0 = 4 * (4 * wave + (lane >> 4));    // first of this lane's 4 outputs
    const int jm = j0 + (cp & 3), qr = cp >> 2;     // unit / gate (i, f, g, o) of this lane in the gate stage
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* stage = smem;                            // [2][LSTMB_CH][LSTMB_ROW]
    float* gl = smem + 2 * LSTMB_CH * LSTMB_ROW;    // [2][LSTMB_GL]
    f32x2 ut[4][16];   // ut[a][p] = U[j0 + (a ^ (cp & 3))][32cp + 2p .. +1]
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int p = 0; p < 16; ++p) {
            const int ar = a ^ (cp & 3);
            ut[a][p].x = U[(size_t)(j0 + ar) * LSTM_G + 32 * cp + 2 * p];
            ut[a][p].y = U[(size_t)(j0 + ar) * LSTM_G + 32 * cp + 2 * p + 1];
            if constexpr (DROP) {      // diag(rm) U: row j0 + ar, the output accumulator a sums
                const float m = (dir ? rm_b : rm_f)[(size_t)b * LSTM_U + j0 + ar];
                ut[a][p].x *= m;
                ut[a][p].y *= m;
            }
        }
    // BPTT step s is time t = S-1-s (dir 0) or s (dir 1); c_prev(t) = c[t-1] (dir 0) / c[t+1] (dir 1), zero outside the sequence
    const int cshift = dir ? 1 : -1;
    const int nchunks = (S + LSTMB_CH - 1) / LSTMB_CH;
    float4 stg[4];
    auto chunk_rows = [&](int c, int& n, int& tlo) {
        const int s0 = c * LSTMB_CH;
        n = min(LSTMB_CH, S - s0);
        tlo = dir ? s0 : S - s0 - n;
    };
    // each staging slot (tid, uu) always reads the same array: (base pointer, row stride, time shift, chunk row) resolved ONCE (gru_bwd_kernel)
    const float* sbase[4];
    int sstride[4], sshift[4], srow[4];
#pragma unroll
    for (int uu = 0; uu < 4; ++uu) {
        const int idx = tid + 512 * uu;           // float4 slot: row = idx / 224, col4 = idx % 224
        const int row = idx / (LSTMB_ROW / 4), c4 = idx - row * (LSTMB_ROW / 4);
        srow[uu] = row;                            // rows >= LSTMB_CH never pass the `row < n` test
        sshift[uu] = 0;
        if (c4 < 32) { sbase[uu] = dO + c4 * 4; sstride[uu] = LSTM_U; }
        else if (c4 < 160) { sbase[uu] = sv + (c4 - 32) * 4; sstride[uu] = LSTM_G; }
        else if (c4 < 192) { sbase[uu] = Cs + (c4 - 160) * 4; sstride[uu] = LSTM_U; }
        else { sbase[uu] = Cs + (c4 - 192) * 4; sstride[uu] = LSTM_U; sshift[uu] = cshift; }
    }
    unsigned okmask = 0;
    auto issue = [&](int c) {
        int n, tlo;
        chunk_rows(c, n, tlo);
        okmask = 0;
#pragma unroll
        for (int uu = 0; uu < 4; ++uu) {
            const int tt = tlo + srow[uu] + sshift[uu];
            const bool ok = (srow[uu] < n) && (tt >= 0) && (tt < S);
            okmask |= (ok ? 1u : 0u) << uu;
            stg[uu] = *reinterpret_cast<const float4*>(sbase[uu] + (size_t)(ok ? tt : 0) * sstride[uu]);   // always in bounds
        }
    };
    auto commit = [&](int buf) {
#pragma unroll
        for (int uu = 0; uu < 4; ++uu) {
            const int idx = tid + 512 * uu;
            const float4 v = ((okmask >> uu) & 1u) ? stg[uu] : make_float4(0.f, 0.f, 0.f, 0.f);
            if (idx < LSTMB_CH * (LSTMB_ROW / 4)) reinterpret_cast<float4*>(stage + buf * LSTMB_CH * LSTMB_ROW)[idx] = v;
        }
    };
    issue(0);
    commit(0);
    __syncthreads();
    float carry = 0.f, dcc = 0.f;    // dh_c and dc_c of unit jm
    int step = 0;
    const int cidx = qr * LSTM_U + jm;
    const int gl_slot = 36 * (cidx / 32) + cidx % 32;
    const unsigned c_off = 4u * cidx;
    float k_do = 0.f, k_a = 0.f, k_c = 0.f, k_h = 0.f, k_f = 0.f;
    // gate by 0 / 1 lane masks: plain multiply-adds, no exec-mask region in the step (gru_bwd_kernel's pre())
    const float m_i = qr == 0 ? 1.f : 0.f, m_f = qr == 1 ? 1.f : 0.f, m_g = qr == 2 ? 1.f : 0.f, m_o = qr == 3 ? 1.f : 0.f;
    auto pre = [&](const float* sbuf, int row) {
        const float* rp = sbuf + row * LSTMB_ROW;
        k_do = rp[jm];
        const float4 sg4 = *reinterpret_cast<const float4*>(rp + 128 + 4 * jm);   // saved activations [unit][i f g o]
        const float gi = sg4.x, gf = sg4.y, gg = sg4.z, go = sg4.w, tc = tanh_(rp[640 + jm]), cprev = rp[768 + jm];
        k_a = go * (1.f - tc * tc);
        const float ki = gg * gi * (1.f - gi), kf = cprev * gf * (1.f - gf), kg = gi * (1.f - gg * gg);
        k_c = fmaf(m_i, ki, fmaf(m_f, kf, m_g * kg));
        k_h = m_o * (tc * go * (1.f - go));
        k_f = gf;
    };
    {
        int n0, tlo0;
        chunk_rows(0, n0, tlo0);
        pre(stage, dir ? 0 : n0 - 1);
    }
    for (int c = 0; c < nchunks; ++c) {
        int n, tlo;
        chunk_rows(c, n, tlo);
        issue(min(c + 1, nchunks - 1));   // unconditional: see gru_fwd_kernel's chunk loop
        const float* sb = stage + (c & 1) * LSTMB_CH * LSTMB_ROW;
        float* gw = nullptr;
        auto part1 = [&](int i) {   // gate gradients of step i -> LDS vector + global
            const int row = dir ? i : n - 1 - i;
            const int t = tlo + row;
            const float dh = k_do + carry;
            const float dc = fmaf(dh, k_a, dcc);
            const float dz = fmaf(dc, k_c, dh * k_h);
            dcc = dc * k_f;
            gw = gl + (step & 1) * LSTMB_GL;
            gw[gl_slot] = dz;
            __builtin_amdgcn_sched_barrier(0);
            // uniform base + 32-bit byte offset: an SGPR-base store
            *reinterpret_cast<float*>(reinterpret_cast<char*>(dgx) + ((unsigned)t * (LSTM_G * 4u) + c_off)) = dz;
        };
        auto part2 = [&]() {        // dh_c = dz U^T
            const float* gp = gw + 36 * cp;
            f32x2 s2[4] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
#pragma unroll
            for (int c4 = 0; c4 < 8; ++c4) {
                const float4 gv = *reinterpret_cast<const float4*>(gp + 4 * c4);
                const f32x2 g01 = {gv.x, gv.y}, g23 = {gv.z, gv.w};
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    s2[a] = pk_fma(g01, ut[a][2 * c4], s2[a]);
                    s2[a] = pk_fma(g23, ut[a][2 * c4 + 1], s2[a]);
                }
            }
            // accumulator a holds output (cp & 3) ^ a: fold over the quad (3 adds), then over the four quads of the row (2 adds)
            const float a0 = (s2[0].x + s2[0].y) + dpp<0xB1 /*quad_perm [1,0,3,2]*/>(s2[1].x + s2[1].y);
            const float a2 = (s2[2].x + s2[2].y) + dpp<0xB1>(s2[3].x + s2[3].y);
            float mine = a0 + dpp<0x4E /*quad_perm [2,3,0,1]*/>(a2);
            mine += dpp<0x128 /*row_ror:8*/>(mine);
            mine += dpp<0x124 /*row_ror:4*/>(mine);
            carry = mine;
            ++step;
        };
        for (int i = 0; i < n - 1; ++i) {
            part1(i);
            lds_barrier();   // LDS-only barrier: never wait for the dgx stores
            pre(sb, dir ? i + 1 : n - 2 - i);
            part2();
        }
        part1(n - 1);
        commit((c + 1) & 1);  // the only wait on the staged loads
        lds_barrier();
        {
            // first step of the next chunk (its rows were committed just above); after the last chunk: the same rows again, unused
            int n2, tlo2;
            chunk_rows(min(c + 1, nchunks - 1), n2, tlo2);
            pre(stage + ((c + 1) & 1) * LSTMB_CH * LSTMB_ROW, dir ? 0 : n2 - 1);
        }
        part2();
    }
}

}  // namespace

// gx_b == nullptr: one direction (grid B).  SAVE form iff c_f is given.  rm_f: the DROP form (training: c and sv are given)
int launch_lstm_fwd(hipStream_t st, const float* gx_f, const float* gx_b, const float* U_f, const float* U_b, float* h_f, float* h_b,
                    float* c_f, float* c_b, float* sv_f, float* sv_b, int B, int S, const float* rm_f, const float* rm_b) {
    const int ndir = gx_b ? 2 : 1;
    if (rm_f && (!c_f || !sv_f || (ndir == 2 && !rm_b))) return -1;
    const size_t smem = (size_t)(2 * LSTMF_CH * LSTM_G + 2 * LSTM_HL) * sizeof(float);
    auto kern = rm_f ? lstm_fwd_kernel<true, true> : c_f ? lstm_fwd_kernel<true> : lstm_fwd_kernel<false>;
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) != hipSuccess) return -1;
    hipLaunchKernelGGL(kern, dim3(ndir * B), dim3(512), smem, st, gx_f, gx_b, U_f, U_b, h_f, h_b, c_f, c_b, sv_f, sv_b, S, ndir, rm_f, rm_b);
    return 0;
}

int launch_lstm_bwd(hipStream_t st, const float* dh_f, const float* dh_b, const float* c_f, const float* c_b, const float* sv_f,
                    const float* sv_b, const float* U_f, const float* U_b, float* dgx_f, float* dgx_b, int B, int S, const float* rm_f,
                    const float* rm_b) {
    const int ndir = dh_b ? 2 : 1;
    if (rm_f && ndir == 2 && !rm_b) return -1;
    const size_t smem = (size_t)(2 * LSTMB_CH * LSTMB_ROW + 2 * LSTMB_GL) * sizeof(float);
    auto kern = rm_f ? lstm_bwd_kernel<true> : lstm_bwd_kernel<false>;
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) != hipSuccess) return -1;
    hipLaunchKernelGGL(kern, dim3(ndir * B), dim3(512), smem, st, dh_f, dh_b, c_f, c_b, sv_f, sv_b, U_f, U_b, dgx_f, dgx_b, S, ndir, rm_f, rm_b);
    return 0;
}
