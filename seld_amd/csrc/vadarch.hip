// vadarch.hip — the head of models.vad_architecture (reference models.py:98-102): Dense(last_unit, sigmoid) on [rows, D] with last_unit = U
// from 1 to 8, and its backward from the binary cross-entropy of seld_vad_bce.  A row-dot of U columns is no work for a 32-column MFMA tile:
// these kernels are exact fp32 FMA chains that read x once.  C ABI "seld_vadarch_*" under the seld_m_* contract (module_ops.hip): fp32 device
// tensors, asynchronous on the caller's stream, no allocation, no atomics, every sum in an order the shape alone fixes.
//
// seld_vadarch_head_fwd — G lanes of one wave own a row (G = the power of two that covers D / 4, at most 64: a function of D alone).  Element d
//   belongs to lane (d / 4) % G, which adds its elements in ascending d into one chain per column; an xor butterfly over the G lanes (DPP
//   inside a row of 16, two shuffles above) joins the chains — both sides of every stage add the same two numbers, so the lanes agree.  The
//   vector form (float4 where D % 4 == 0 and x is aligned) loads the same elements the scalar form does: the same bits.
// seld_vadarch_head_bwd — stage one, workgroup (d tile, row chunk): 256 threads = TD lanes along d (four columns of x each) x 256 / TD row
//   lanes.  Per tile of 32 rows the workgroup forms dz (and, in the first d tile, the loss terms and db) in LDS; a thread then walks its rows
//   in ascending order: dx = dz w^T is written, x dz joins the thread's dw chains.  The row lanes' chains are added in LDS in ascending lane
//   order into the chunk's partial.  Stage two adds the chunks' partials in ascending order (dw: one thread per element; loss: the fixed
//   tree of seld_vad_bce; db: one thread per column).
#include "common.h"

namespace {

constexpr int VA_MAX_U = 8;
constexpr int VA_TILE_ROWS = 32;       // rows whose dz a backward workgroup holds in LDS at a time
constexpr int VA_MAX_CHUNKS = 1024;    // row chunks (= partials per element) of the backward, at most
constexpr float VA_EPS = 1e-7f;        // tf.keras.backend.epsilon()

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// lanes per row of the forward: a power of two, D alone decides
int fwd_group(int D) {
    const int need = (D + 3) / 4;
    int G = 1;
    while (G < 64 && G < need) G *= 2;
    return G;
}

// lanes along d of a backward workgroup (each owns four columns): a power of two up to 256, D alone decides
int bwd_td(int D) {
    const int need = (D + 3) / 4;
    int TD = 1;
    while (TD < 256 && TD < need) TD *= 2;
    return TD;
}

// chunks of the backward and rows per chunk: rows alone decides.  The count never falls as rows grows (a model sizes its scratch for its
// largest batch and runs smaller ones), so past the cap the last chunks of a launch may hold no row: they write zero partials
void bwd_chunks(int64_t rows, int64_t& RC, int& NC) {
    const int64_t nc = (rows + VA_TILE_ROWS - 1) / VA_TILE_ROWS;
    NC = (int)(nc < VA_MAX_CHUNKS ? nc : VA_MAX_CHUNKS);
    RC = (rows + NC - 1) / NC;
}

// the sum over the G lanes (a power of two, aligned) that hold a row's chains, in every one of them
__device__ __forceinline__ float group_sum(float v, int G) {
    if (G >= 2) v += dpp<0xB1 /*quad_perm [1,0,3,2]*/>(v);
    if (G >= 4) v += dpp<0x4E /*quad_perm [2,3,0,1]*/>(v);
    if (G >= 8) v += dpp<0x141 /*row_half_mirror*/>(v);      // the quads agree inside: lane l takes 7 - l, the other quad of its eight
    if (G >= 16) v += dpp<0x140 /*row_mirror*/>(v);          // lane l takes 15 - l, the other eight of its row
    if (G >= 32) v += __shfl_xor(v, 16, 64);
    if (G >= 64) v += __shfl_xor(v, 32, 64);
    return v;
}

template <int U>
__global__ __launch_bounds__(256) void head_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                                       float* __restrict__ p, int64_t rows, int D, int G, int vec) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rpw = 64 / G;
    const int64_t r = ((int64_t)blockIdx.x * 4 + wave) * rpw + lane / G;
    const int gl = lane & (G - 1);
    const bool active = r < rows;
    float acc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) acc[u] = 0.f;
    if (active) {
        const float* xr = x + (size_t)r * D;
        for (int64_t d0 = (int64_t)gl * 4; d0 < D; d0 += (int64_t)G * 4) {
            float xv[4];
            if (vec) {
                const float4 t = *reinterpret_cast<const float4*>(xr + d0);
                xv[0] = t.x; xv[1] = t.y; xv[2] = t.z; xv[3] = t.w;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) xv[i] = d0 + i < D ? xr[d0 + i] : 0.f;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (d0 + i < D) {
                    const float* wr = w + (size_t)(d0 + i) * U;
#pragma unroll
                    for (int u = 0; u < U; ++u) acc[u] = fmaf(xv[i], wr[u], acc[u]);
                }
            }
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) acc[u] = group_sum(acc[u], G);
    if (active && gl == 0) {
#pragma unroll
        for (int u = 0; u < U; ++u) p[(size_t)r * U + u] = 1.f / (1.f + expf(-(acc[u] + b[u])));
    }
}

// the workgroup's 256 values -> their sum, by a fixed tree (seld_vad_bce's)
__device__ __forceinline__ float tree_sum256(float v, float* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    return red[0];
}

// part [NC][D * U], lossp [NC], dbp [NC][U]: the chunks' partial sums
template <int U>
__global__ __launch_bounds__(256) void head_bwd_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ p,
                                                       const float* __restrict__ y, float* __restrict__ dx, float* __restrict__ part,
                                                       float* __restrict__ lossp, float* __restrict__ dbp, int64_t rows, int D, int TD,
                                                       int64_t RC, float gscale, int vec) {
    __shared__ float dzs[VA_TILE_ROWS * U];
    __shared__ float red[256 * 4 * U];
    const int tid = threadIdx.x;
    const int td = tid & (TD - 1), j = tid / TD, TR = 256 / TD;
    const int64_t d0 = ((int64_t)blockIdx.x * TD + td) * 4;
    const int c = blockIdx.y;
    const int64_t r_begin = (int64_t)c * RC;
    const int64_t r_end = r_begin + RC < rows ? r_begin + RC : rows;      // r_end <= r_begin: a chunk without rows, its partials are 0
    const float lo = VA_EPS, hi = 1.f - VA_EPS;
    float wv[4][U], acc[4][U];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int u = 0; u < U; ++u) {
            wv[i][u] = d0 + i < D ? w[(size_t)(d0 + i) * U + u] : 0.f;
            acc[i][u] = 0.f;
        }
    float lacc = 0.f, dbacc = 0.f;
    for (int64_t t0 = r_begin; t0 < r_end; t0 += VA_TILE_ROWS) {
        const int nr = (int)(r_end - t0 < VA_TILE_ROWS ? r_end - t0 : VA_TILE_ROWS);
        if (tid < nr * U) {      // element (row t0 + tid / U, column tid % U): a thread keeps its column over the tiles
            const size_t e = (size_t)t0 * U + tid;
            const float pv = p[e], yv = y[e];
            const float pc = fminf(fmaxf(pv, lo), hi);
            const float a = pc + VA_EPS, q = 1.f - pc + VA_EPS;
            const float dp = (pv < lo || pv > hi) ? 0.f : gscale * ((1.f - yv) / q - yv / a);
            const float dz = dp * (pv * (1.f - pv));
            dzs[tid] = dz;
            if (blockIdx.x == 0) {      // the first column tile alone keeps the loss terms and db
                lacc -= yv * logf(a) + (1.f - yv) * logf(q);
                dbacc += dz;
            }
        }
        __syncthreads();
        if (d0 < D) {
            for (int rl = j; rl < nr; rl += TR) {
                const size_t off = (size_t)(t0 + rl) * D + d0;
                float xv[4], dzr[U];
#pragma unroll
                for (int u = 0; u < U; ++u) dzr[u] = dzs[rl * U + u];
                if (vec) {
                    const float4 t = *reinterpret_cast<const float4*>(x + off);
                    xv[0] = t.x; xv[1] = t.y; xv[2] = t.z; xv[3] = t.w;
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) xv[i] = d0 + i < D ? x[off + i] : 0.f;
                }
                float g[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    g[i] = dzr[0] * wv[i][0];
#pragma unroll
                    for (int u = 1; u < U; ++u) g[i] = fmaf(dzr[u], wv[i][u], g[i]);
#pragma unroll
                    for (int u = 0; u < U; ++u) acc[i][u] = fmaf(xv[i], dzr[u], acc[i][u]);
                }
                if (dx) {
                    if (vec) {
                        *reinterpret_cast<float4*>(dx + off) = make_float4(g[0], g[1], g[2], g[3]);
                    } else {
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if (d0 + i < D) dx[off + i] = g[i];
                    }
                }
            }
        }
        __syncthreads();
    }
    // the row lanes' chains of one (d, u), added in ascending lane order
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int u = 0; u < U; ++u) red[tid * (4 * U) + i * U + u] = acc[i][u];
    __syncthreads();
    if (j == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (d0 + i < D) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    float s = 0.f;
                    for (int jj = 0; jj < TR; ++jj) s += red[(jj * TD + td) * (4 * U) + i * U + u];
                    part[(size_t)c * ((size_t)D * U) + (size_t)(d0 + i) * U + u] = s;
                }
            }
        }
    }
    if (blockIdx.x != 0) return;
    __syncthreads();
    red[256 + tid] = dbacc;      // threads past 32 U hold 0
    __syncthreads();
    if (tid < U) {
        float s = 0.f;
        for (int rl = 0; rl < VA_TILE_ROWS; ++rl) s += red[256 + rl * U + tid];
        dbp[c * U + tid] = s;
    }
    const float tot = tree_sum256(lacc, red);
    if (tid == 0) lossp[c] = tot;
}

// blocks 0 .. nb - 1: dw; block nb: the loss and db
__global__ __launch_bounds__(256) void head_bwd_final_kernel(const float* __restrict__ part, const float* __restrict__ lossp,
                                                             const float* __restrict__ dbp, float* __restrict__ dw, float* __restrict__ db,
                                                             float* __restrict__ loss, int NC, int64_t DU, int U, unsigned nb, float scale) {
    __shared__ float red[256];
    if (blockIdx.x < nb) {
        const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
        if (e >= DU) return;
        float s = 0.f;
        for (int c = 0; c < NC; ++c) s += part[(size_t)c * DU + e];
        dw[e] = s;
        return;
    }
    if ((int)threadIdx.x < U) {
        float s = 0.f;
        for (int c = 0; c < NC; ++c) s += dbp[c * U + threadIdx.x];
        db[threadIdx.x] = s;
    }
    float acc = 0.f;
    for (int c = threadIdx.x; c < NC; c += 256) acc += lossp[c];
    const float tot = tree_sum256(acc, red);
    if (threadIdx.x == 0) *loss = scale * tot;
}

template <int U>
void launch_fwd(hipStream_t st, const float* x, const float* w, const float* b, float* p, int64_t rows, int D, int G, unsigned grid, int vec) {
    hipLaunchKernelGGL(head_fwd_kernel<U>, dim3(grid), dim3(256), 0, st, x, w, b, p, rows, D, G, vec);
}

template <int U>
void launch_bwd(hipStream_t st, dim3 grid, const float* x, const float* w, const float* p, const float* y, float* dx, float* part, float* lossp,
                float* dbp, int64_t rows, int D, int TD, int64_t RC, float gscale, int vec) {
    hipLaunchKernelGGL(head_bwd_kernel<U>, grid, dim3(256), 0, st, x, w, p, y, dx, part, lossp, dbp, rows, D, TD, RC, gscale, vec);
}

#define VA_DISPATCH(U, CALL)                                                                                                               \
    switch (U) {                                                                                                                           \
        case 1: CALL(1); break;                                                                                                            \
        case 2: CALL(2); break;                                                                                                            \
        case 3: CALL(3); break;                                                                                                            \
        case 4: CALL(4); break;                                                                                                            \
        case 5: CALL(5); break;                                                                                                            \
        case 6: CALL(6); break;                                                                                                            \
        case 7: CALL(7); break;                                                                                                            \
        default: CALL(8); break;                                                                                                           \
    }

}  // namespace

extern "C" {

int seld_vadarch_head_fwd(const float* x, const float* w, const float* b, float* p, int64_t rows, int D, int U, void* stream) {
    if (!x || !w || !b || !p || rows < 1 || D < 1 || U < 1) return SELD_ERR_INVALID;
    if (U > VA_MAX_U) return SELD_ERR_UNSUPPORTED;
    const int G = fwd_group(D);
    const int64_t rpb = 4 * (64 / G);
    const int64_t grid = (rows + rpb - 1) / rpb;
    if (grid > 0x7fffffff) return SELD_ERR_UNSUPPORTED;
    const int vec = D % 4 == 0 && al16(x);
#define VA_FWD(UU) launch_fwd<UU>((hipStream_t)stream, x, w, b, p, rows, D, G, (unsigned)grid, vec)
    VA_DISPATCH(U, VA_FWD)
#undef VA_FWD
    return ok();
}

int64_t seld_vadarch_head_bwd_scratch(int64_t rows, int D, int U) {
    if (rows < 1 || D < 1 || U < 1 || U > VA_MAX_U) return -1;
    int64_t RC;
    int NC;
    bwd_chunks(rows, RC, NC);
    return (int64_t)NC * ((int64_t)D * U + 1 + U);
}

int seld_vadarch_head_bwd(const float* x, const float* w, const float* p, const float* y, float* loss, float* dx, float* dw, float* db,
                          float* scratch, int64_t rows, int D, int U, float weight, void* stream) {
    if (!x || !w || !p || !y || !loss || !dw || !db || !scratch || rows < 1 || D < 1 || U < 1) return SELD_ERR_INVALID;
    if (U > VA_MAX_U) return SELD_ERR_UNSUPPORTED;
    int64_t RC;
    int NC;
    bwd_chunks(rows, RC, NC);
    const int TD = bwd_td(D);
    const int64_t DU = (int64_t)D * U;
    const int64_t tiles = ((int64_t)D + (int64_t)TD * 4 - 1) / ((int64_t)TD * 4);
    const int64_t nb = (DU + 255) / 256;
    float* part = scratch;
    float* lossp = scratch + (size_t)NC * DU;
    float* dbp = lossp + NC;
    const float scale = weight / (float)((double)rows * U);
    const int vec = D % 4 == 0 && al16(x) && (!dx || al16(dx));
#define VA_BWD(UU) launch_bwd<UU>((hipStream_t)stream, dim3((unsigned)tiles, (unsigned)NC), x, w, p, y, dx, part, lossp, dbp, rows, D, TD, RC, scale, vec)
    VA_DISPATCH(U, VA_BWD)
#undef VA_BWD
    hipLaunchKernelGGL(head_bwd_final_kernel, dim3((unsigned)nb + 1), dim3(256), 0, (hipStream_t)stream, part, lossp, dbp, dw, db, loss, NC, DU, U,
                       (unsigned)nb, scale);
    return ok();
}

}  // extern "C"
