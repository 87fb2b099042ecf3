// trainv2.hip — the per-step device work of the reference's second training script (trainv2.py:23-56) that is not the model:
//   losses_v2_kernel       class-weighted BCE (K.binary_crossentropy * cls_weights) or focal loss (losses.py:29-34) with optional label
//                          smoothing + losses.MMSE_with_cls_weights (losses.py:16-26): loss values and the gradients w.r.t. the heads'
//                          PRE-activations, one pass
//   v2_unit_scale_kernel   utils.adaptive_clip_grad (utils.py:86-96) behind the L2 kernel regulariser (utils.py:343-350): the clip factor of
//                          every unit of every variable in ONE launch
//   adabelief_kernel       utils.AdaBelief (utils.py:99-194, amsgrad=False) over the flat buffers, regulariser and clip folded in
//   swa_kernel             swa.SWA.update_swa_weights (swa.py:25-32)
// and the C ABI around them (include/seld_hip.h: seld_k_losses_v2, seld_k_reg_agc_adabelief, seld_train_fwd_bwd_v2, seld_set_regularized,
// seld_v2_opt_step, seld_swa_*; for composed models the stream operators seld_v2_losses, seld_v2_plan_*, seld_v2_opt, seld_v2_swa).
// Nothing here is library-wide state: the tables live in the context, or in the plan a composed model owns.
#include "ctx.h"

#include <algorithm>
#include <math.h>
#include <stdint.h>
#include <vector>

#define V2_EPS 1e-7f      // K.epsilon() of K.binary_crossentropy, eps of losses.focal_loss

struct V2W { float w[SELD_V2_MAX_CLASSES]; };      // the class weights, a kernel argument by value

// kernel arguments are read with compile-time indices only (a run-time index would move the struct to scratch): thread i copies w[i] to LDS
__device__ __forceinline__ void v2_weights_to_lds(const V2W& W, float* wl) {
#pragma unroll
    for (int i = 0; i < SELD_V2_MAX_CLASSES; ++i)
        if ((int)threadIdx.x == i) wl[i] = W.w[i];
    __syncthreads();
}

// sum([m|m|m]) of losses.MMSE_with_cls_weights, m[r, c] = round(|y[r, :, c]|^2) * w[c]: one workgroup, thread t adds the rows t, t + 1024, ...
// in order (double), then a fixed tree over the threads — the same bits every run.  Replaces launch_mmse_den's three launches.
__global__ __launch_bounds__(1024) void mmse_den_v2_kernel(const float* __restrict__ y_doa, V2W W, float* __restrict__ den, int rows, int nc) {
    __shared__ double red[1024];
    __shared__ float wl[SELD_V2_MAX_CLASSES];
    v2_weights_to_lds(W, wl);
    double s = 0.0;
    for (int r = threadIdx.x; r < rows; r += 1024) {
        const float* y = y_doa + (size_t)r * 3 * nc;
        float a = 0.f;
        for (int c = 0; c < nc; ++c) {
            const float x0 = y[c], x1 = y[nc + c], x2 = y[2 * nc + c];
            a += 3.f * (rintf(x0 * x0 + x1 * x1 + x2 * x2) * wl[c]);
        }
        s += (double)a;
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) den[0] = (float)red[0];
}

// sum over the 4 lanes of a quad (every lane gets the sum)
__device__ __forceinline__ float v2_quad_sum(float v) {
    v += dpp_quad_xor1(v);
    v += dpp_quad_xor2(v);
    return v;
}

// The layout of losses_kernel (loss_adam.hip): four lanes per row (lane q takes the columns q, q + 4, ...), 64 rows per workgroup, the two
// sums per workgroup reduced in a fixed order (quad -> row order in LDS, double) into blockpart[block][2]; losses_v2_finalize_kernel adds those
// in block order.  sed_loss SELD_SED_BCE: blockpart[.][0] = sum bce(t, p) w[c]; SELD_SED_FOCAL: sum of the focal terms (the finalize multiplies
// by mean(w): the reference multiplies the scalar focal loss by the weight row and takes the mean).  coef_sed = d objective / d (that sum).
__global__ __launch_bounds__(256) void losses_v2_kernel(const float* __restrict__ sed, const float* __restrict__ doa, const float* __restrict__ y_sed,
                                                        const float* __restrict__ y_doa, V2W W, int sed_loss, float ls, float alpha, float gamma,
                                                        float coef_sed, float w_doa, const float* __restrict__ den_dev, float* __restrict__ dsed_pre,
                                                        float* __restrict__ ddoa_pre, double* __restrict__ blockpart, int rows, int nc, int ld_sed,
                                                        int ld_doa) {
    __shared__ float rs[64][2];
    __shared__ float wl[SELD_V2_MAX_CLASSES];
    v2_weights_to_lds(W, wl);
    const int q = threadIdx.x & 3, rl = threadIdx.x >> 2;
    const int r = min(blockIdx.x * 64 + rl, rows - 1);       // rows past the end recompute the last row and store nothing
    const bool live = blockIdx.x * 64 + rl < rows;
    const float* p = sed + (size_t)r * nc;
    const float* ys = y_sed + (size_t)r * nc;
    float bsum = 0.f;
    for (int c = q; c < nc; c += 4) {
        const float pv = p[c];
        float t = ys[c];
        if (ls > 0.f) t = t * (1.f - ls) + 0.5f * ls;        // trainv2.py:38-39
        const float pc = fminf(fmaxf(pv, V2_EPS), 1.f - V2_EPS);
        const bool pass = (pv >= V2_EPS) && (pv <= 1.f - V2_EPS);      // tf.clip_by_value passes the gradient inside the closed interval
        float term, dldp;
        if (sed_loss == SELD_SED_BCE) {
            const float wc = wl[c];
            term = -(t * logf(pc + V2_EPS) + (1.f - t) * logf(1.f - pc + V2_EPS)) * wc;
            dldp = -(t / (pc + V2_EPS) - (1.f - t) / (1.f - pc + V2_EPS)) * wc;
        } else {
            // -t a (1 - p)^g log p - (1 - t) a p^g log(1 - p) and its derivative in p
            const float om = 1.f - pc, lp = logf(pc), lq = log1pf(-pc);
            float pa, pb, pa1, pb1;                          // (1 - p)^g, p^g, (1 - p)^(g - 1), p^(g - 1)
            if (gamma == 2.f) { pa1 = om; pb1 = pc; }
            else { pa1 = powf(om, gamma - 1.f); pb1 = powf(pc, gamma - 1.f); }
            pa = pa1 * om; pb = pb1 * pc;
            term = -alpha * (t * pa * lp + (1.f - t) * pb * lq);
            dldp = -alpha * (t * (pa / pc - gamma * pa1 * lp) + (1.f - t) * (gamma * pb1 * lq - pb / om));
        }
        bsum += term;
        if (dsed_pre && live) dsed_pre[(size_t)r * ld_sed + c] = coef_sed * (pass ? dldp : 0.f) * pv * (1.f - pv);
    }
    const float* d = doa + (size_t)r * 3 * nc;
    const float* yd = y_doa + (size_t)r * 3 * nc;
    const float den = den_dev[0];
    float dsum = 0.f;
    for (int c = q; c < nc; c += 4) {
        const float x0 = yd[c], x1 = yd[nc + c], x2 = yd[2 * nc + c];
        const float m = rintf(x0 * x0 + x1 * x1 + x2 * x2) * wl[c];
        for (int k = 0; k < 3; ++k) {
            const int i = k * nc + c;
            const float e = yd[i] - d[i];
            dsum += e * e * m;
            if (ddoa_pre && live) ddoa_pre[(size_t)r * ld_doa + i] = w_doa * (-2.f * e * m / den) * (1.f - d[i] * d[i]);
        }
    }
    dsum = v2_quad_sum(dsum);
    bsum = v2_quad_sum(bsum);
    if (q == 0) { rs[rl][0] = live ? bsum : 0.f; rs[rl][1] = live ? dsum : 0.f; }
    __syncthreads();
    if (threadIdx.x < 2) {
        double s = 0.0;
        for (int i = 0; i < 64; ++i) s += (double)rs[i][threadIdx.x];
        blockpart[(size_t)blockIdx.x * 2 + threadIdx.x] = s;
    }
}

// one wave: lane l adds the partials l, l + 64, ... in order, then a fixed xor tree over the lanes
__global__ __launch_bounds__(64) void losses_v2_finalize_kernel(const double* __restrict__ blockpart, int nblocks, double sed_scale,
                                                                const float* __restrict__ den_dev, float* __restrict__ sloss,
                                                                float* __restrict__ dloss) {
    double s0 = 0.0, s1 = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += 64) { s0 += blockpart[2 * i]; s1 += blockpart[2 * i + 1]; }
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) { s0 += __shfl_xor(s0, w); s1 += __shfl_xor(s1, w); }
    if (threadIdx.x) return;
    if (sloss) sloss[0] = (float)(s0 * sed_scale);
    if (dloss) dloss[0] = (float)(s1 / (double)den_dev[0]);
}

static int v2_cfg_ok(const seld_v2_cfg* cfg, int nc) {
    return cfg && nc >= 1 && nc <= SELD_V2_MAX_CLASSES && (cfg->sed_loss == SELD_SED_BCE || cfg->sed_loss == SELD_SED_FOCAL) &&
           cfg->label_smoothing >= 0.f && cfg->label_smoothing < 1.f;
}

// den_dev: 1 float; scratch: loss_scratch_floats(rows) floats (the per-workgroup partials); ld_*: row strides of the two gradient outputs
// (<= 0: nc / 3 nc).  Objective = sloss w_sed + dloss w_doa, both scalars (trainv2.py:44): no `rows` factor as in launch_losses' MSE form.
static void launch_losses_v2(hipStream_t st, const float* sed, const float* doa, const float* y_sed, const float* y_doa, const seld_v2_cfg* cfg,
                             float* den_dev, float* sloss, float* dloss, float* dsed_pre, float* ddoa_pre, float* scratch, int rows, int nc,
                             int ld_sed, int ld_doa) {
    if (ld_sed <= 0) ld_sed = nc;
    if (ld_doa <= 0) ld_doa = 3 * nc;
    V2W W;
    double wmean = 0.0;
    for (int i = 0; i < SELD_V2_MAX_CLASSES; ++i) { W.w[i] = i < nc ? cfg->cls_weights[i] : 0.f; wmean += (double)W.w[i]; }
    wmean /= (double)nc;
    const double inv_n = 1.0 / ((double)rows * (double)nc);
    const double sed_scale = cfg->sed_loss == SELD_SED_FOCAL ? wmean * inv_n : inv_n;
    double* blockpart = reinterpret_cast<double*>(scratch);
    const int nblocks = (rows + 63) / 64;
    hipLaunchKernelGGL(mmse_den_v2_kernel, dim3(1), dim3(1024), 0, st, y_doa, W, den_dev, rows, nc);
    hipLaunchKernelGGL(losses_v2_kernel, dim3(nblocks), dim3(256), 0, st, sed, doa, y_sed, y_doa, W, (int)cfg->sed_loss, cfg->label_smoothing,
                       cfg->focal_alpha, cfg->focal_gamma, (float)((double)cfg->w_sed * sed_scale), cfg->w_doa, den_dev, dsed_pre, ddoa_pre,
                       blockpart, rows, nc, ld_sed, ld_doa);
    hipLaunchKernelGGL(losses_v2_finalize_kernel, dim3(1), dim3(64), 0, st, blockpart, nblocks, sed_scale, den_dev, sloss, dloss);
}

// ------------------------------------------------------------------------------------------------ regulariser + AGC + AdaBelief
// A variable is [rows][cols] with one clip unit per column (launch_agc's mapping of a Keras shape).  One workgroup of v2_unit_scale_kernel
// takes a tile of tc (a power of two <= 64) columns: thread t reads column t % tc of the rows t / tc, t / tc + 256 / tc, ... — consecutive
// lanes read consecutive addresses, a unit's rows are spread over 256 / tc lanes — and the 256 / tc partial sums of a column are added by a
// tree over LDS whose shape depends on tc alone: fixed order, no atomics.
struct V2Tile { int64_t off; int32_t rows, cols, c0, tc, unit0, var; };
// [a, b) of the flat buffers, inside variable `var` (at `off`, `cols` columns, units from unit0); a / b are multiples of 4 except at the
// variable's own ends
struct V2Seg { int64_t a, b, off; int32_t cols, unit0, var, pad; };
#define V2_SEG_ELEMS 4096

__global__ __launch_bounds__(256) void v2_unit_scale_kernel(const float* __restrict__ theta, const float* __restrict__ g, const V2Tile* __restrict__ tiles,
                                                            const int32_t* __restrict__ reg, float l2x2, float clip, float* __restrict__ scale) {
    __shared__ float rp[256], rg[256];
    const V2Tile T = tiles[blockIdx.x];
    const int t = threadIdx.x, col = t & (T.tc - 1), slot = t / T.tc, nslot = 256 / T.tc;
    const int c = T.c0 + col;
    const float k = reg[T.var] ? l2x2 : 0.f;
    float pn = 0.f, gn = 0.f;
    if (c < T.cols)
        for (int r = slot; r < T.rows; r += nslot) {
            const int64_t i = T.off + (int64_t)r * T.cols + c;
            const float w = theta[i], gg = g[i] + k * w;
            pn += w * w;
            gn += gg * gg;
        }
    rp[t] = pn; rg[t] = gn;
    __syncthreads();
    for (int s = 128; s >= T.tc; s >>= 1) {
        if (t < s) { rp[t] += rp[t + s]; rg[t] += rg[t + s]; }
        __syncthreads();
    }
    if (t < T.tc && c < T.cols) {
        pn = sqrtf(rp[t]);
        gn = sqrtf(rg[t]);
        const float max_norm = fmaxf(pn, 1e-3f) * clip;
        scale[T.unit0 + c] = gn < max_norm ? 1.f : max_norm / fmaxf(gn, 1e-6f);
    }
}

struct V2Hyper { float lr_t, b1, b2, eps; };

__device__ __forceinline__ void adabelief_one(float& w, float& g, float& m, float& v, float k, float sc, const V2Hyper& h) {
    const float gp = (g + k * w) * sc;
    const float mi = h.b1 * m + (1.f - h.b1) * gp;
    const float d = gp - mi;                                 // the UPDATED first moment (utils.py:171)
    const float vi = h.b2 * v + (1.f - h.b2) * d * d;
    w = w - h.lr_t * mi / (sqrtf(vi) + h.eps);
    g = gp; m = mi; v = vi;
}

// one workgroup per segment; float4 over the aligned middle of the segment, the (at most 3 + 3) elements at a variable's unaligned ends by
// the first threads one by one.  scale == nullptr: no clip.
__global__ __launch_bounds__(256) void adabelief_kernel(float* __restrict__ theta, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                        const V2Seg* __restrict__ segs, const int32_t* __restrict__ reg, const float* __restrict__ scale,
                                                        float l2x2, V2Hyper h) {
    const V2Seg S = segs[blockIdx.x];
    const float k = reg[S.var] ? l2x2 : 0.f;
    const unsigned cols = (unsigned)S.cols;
    const float* sc = scale ? scale + S.unit0 : nullptr;
    const int64_t au = (S.a + 3) & ~(int64_t)3, bd = S.b & ~(int64_t)3;
    const int64_t a4 = au < S.b ? au : S.b, b4 = bd > a4 ? bd : a4;
    const int t = threadIdx.x;
    for (int e = 0; e < 2; ++e) {
        const int64_t i = e == 0 ? S.a + t : b4 + t;
        if (i < (e == 0 ? a4 : S.b)) {
            const float s1 = sc ? sc[(unsigned)(i - S.off) % cols] : 1.f;
            float w_ = theta[i], g_ = g[i], m_ = m[i], v_ = v[i];
            adabelief_one(w_, g_, m_, v_, k, s1, h);
            theta[i] = w_; g[i] = g_; m[i] = m_; v[i] = v_;
        }
    }
    for (int64_t i = a4 + 4 * t; i < b4; i += 1024) {
        float4 w4 = *reinterpret_cast<const float4*>(theta + i), g4 = *reinterpret_cast<const float4*>(g + i);
        float4 m4 = *reinterpret_cast<const float4*>(m + i), v4 = *reinterpret_cast<const float4*>(v + i);
        float s4[4] = {1.f, 1.f, 1.f, 1.f};
        if (sc) {
            unsigned c = (unsigned)(i - S.off) % cols;
#pragma unroll
            for (int j = 0; j < 4; ++j) { s4[j] = sc[c]; c = c + 1 >= cols ? 0 : c + 1; }
        }
        adabelief_one(w4.x, g4.x, m4.x, v4.x, k, s4[0], h);
        adabelief_one(w4.y, g4.y, m4.y, v4.y, k, s4[1], h);
        adabelief_one(w4.z, g4.z, m4.z, v4.z, k, s4[2], h);
        adabelief_one(w4.w, g4.w, m4.w, v4.w, k, s4[3], h);
        *reinterpret_cast<float4*>(theta + i) = w4; *reinterpret_cast<float4*>(g + i) = g4;
        *reinterpret_cast<float4*>(m + i) = m4; *reinterpret_cast<float4*>(v + i) = v4;
    }
}

namespace {
struct V2Host { std::vector<V2Tile> tiles; std::vector<V2Seg> segs; int nunits = 0; };

// tiles and segments of n_vars variables laid out in a flat buffer of n floats; false: a variable is empty, out of the buffer or overlaps
// its predecessor
bool v2_build(int n_vars, const int64_t* off, const int32_t* rows, const int32_t* cols, int64_t n, V2Host& H) {
    int64_t prev_end = 0, units = 0;
    for (int i = 0; i < n_vars; ++i) {
        if (rows[i] < 1 || cols[i] < 1 || off[i] < prev_end) return false;
        const int64_t size = (int64_t)rows[i] * cols[i], end = off[i] + size;
        if (size >= ((int64_t)1 << 31) || end > n || units + cols[i] >= ((int64_t)1 << 31)) return false;
        // columns per tile: up to 64 (a 256-byte row piece per wave); tall variables take 16 (64 bytes) so that more workgroups share the rows
        const int want = std::min<int>(cols[i], rows[i] > 512 ? 16 : 64);
        int tc = 1;
        while (tc < want) tc <<= 1;
        for (int c0 = 0; c0 < cols[i]; c0 += tc) H.tiles.push_back(V2Tile{off[i], rows[i], cols[i], c0, tc, (int32_t)units, i});
        for (int64_t a = off[i]; a < end;) {
            const int64_t b = std::min<int64_t>(end, (a / V2_SEG_ELEMS + 1) * V2_SEG_ELEMS);
            H.segs.push_back(V2Seg{a, b, off[i], cols[i], (int32_t)units, i, 0});
            a = b;
        }
        units += cols[i];
        prev_end = end;
    }
    H.nunits = (int)units;
    return !H.tiles.empty();
}

// launch_agc's mapping of a Keras shape to [rows][cols] (utils.unitwise_norm, utils.py:71-83)
void v2_rows_cols(int rank, const int64_t* shape, int32_t* rows, int32_t* cols) {
    if (rank <= 1) { *rows = (int32_t)shape[0]; *cols = 1; }
    else if (rank == 2) { *rows = (int32_t)shape[0]; *cols = (int32_t)shape[1]; }
    else if (rank == 3) { *rows = (int32_t)shape[0]; *cols = (int32_t)(shape[1] * shape[2]); }
    else { *rows = (int32_t)(shape[0] * shape[1] * shape[2]); *cols = (int32_t)shape[3]; }
}

double v2_lr_t(float lr, float beta1, float beta2, int64_t step) {
    const double t = (double)step;
    return (double)lr * sqrt(1.0 - pow((double)beta2, t)) / (1.0 - pow((double)beta1, t));
}

// the two launches of the optimizer stage, whatever the number of variables
void launch_v2_opt(hipStream_t st, float* theta, float* g, float* m, float* v, const V2Tile* tiles, int ntiles, const V2Seg* segs, int nsegs,
                   const int32_t* reg, float* scale, float lr_t, float beta1, float beta2, float eps, float l2, float clip_factor) {
    const bool agc = clip_factor > 0.f;
    if (agc) hipLaunchKernelGGL(v2_unit_scale_kernel, dim3(ntiles), dim3(256), 0, st, theta, g, tiles, reg, 2.f * l2, clip_factor, scale);
    hipLaunchKernelGGL(adabelief_kernel, dim3(nsegs), dim3(256), 0, st, theta, g, m, v, segs, reg, agc ? scale : nullptr, 2.f * l2,
                       V2Hyper{lr_t, beta1, beta2, eps});
}
}  // namespace

// seld_create: the device tables of the context's trainable variables (flags: none regularised)
int v2_tables_create(seld_ctx* c) {
    const int nv = (int)c->tr.size();
    std::vector<int64_t> off(nv);
    std::vector<int32_t> rows(nv), cols(nv), reg(nv, 0);
    for (int i = 0; i < nv; ++i) { off[i] = c->tr[i].off; v2_rows_cols(c->tr[i].rank, c->tr[i].shape, &rows[i], &cols[i]); }
    V2Host H;
    if (!v2_build(nv, off.data(), rows.data(), cols.data(), c->nparam, H)) return fail(c, SELD_ERR_INVALID, "trainv2: variable table");
    V2Tile* tiles = nullptr; V2Seg* segs = nullptr;
    int rc;
    if ((rc = dalloc(c, &tiles, H.tiles.size())) || (rc = dalloc(c, &segs, H.segs.size())) || (rc = dalloc(c, &c->v2.reg, (size_t)nv)) ||
        (rc = dalloc(c, &c->v2.scale, (size_t)H.nunits)))
        return rc;
    HIPCHK(c, hipMemcpy(tiles, H.tiles.data(), H.tiles.size() * sizeof(V2Tile), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(segs, H.segs.data(), H.segs.size() * sizeof(V2Seg), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->v2.reg, reg.data(), (size_t)nv * sizeof(int32_t), hipMemcpyHostToDevice));
    c->v2.tiles = tiles; c->v2.segs = segs; c->v2.ntiles = (int)H.tiles.size(); c->v2.nsegs = (int)H.segs.size();
    return 0;
}

// the loss stage of seld_train_fwd_bwd_v2: run_losses (api.hip) with the v2 kernels.  The scalars are finalized here, on the main stream:
// backward_impl's deferred finalize belongs to the v1 kernels' partials.
static int run_losses_v2(seld_ctx* c, const float* y_sed, const float* y_doa, const seld_v2_cfg* cfg, float* sloss, float* dloss) {
    hipStream_t st = c->stream;
    const int rows = c->B * c->S, nc = c->arch.n_classes;
    float* sl = sloss ? sloss : c->loss_out;
    float* dl = dloss ? dloss : c->loss_out + 4;
    const bool lin = heads_lin(c);
    const int n0 = c->heads[0].layers.back().out, nt = n0 + c->heads[1].layers.back().out;
    float* dsed = lin ? c->dy_all : c->heads[0].layers.back().dy;
    float* ddoa = lin ? c->dy_all + n0 : c->heads[1].layers.back().dy;
    launch_losses_v2(st, c->heads[0].layers.back().y, c->arch.output_coupling ? c->doa_v1 : c->heads[1].layers.back().y, y_sed, y_doa, cfg, c->den_dev,
                     sl, dl, dsed, ddoa, c->loss_scratch, rows, nc, lin ? nt : 0, lin ? nt : 0);
    // seldnet_v1: the losses left d / d(doa sed) in the DOA slot; through the product to the two heads' pre-activations
    if (c->arch.output_coupling)
        launch_v1_couple_bwd(st, c->heads[0].layers.back().y, c->heads[1].layers.back().y, dsed, lin ? nt : n0, ddoa, lin ? nt : nt - n0, rows, nc);
    c->fin_sl = nullptr;
    return check_launch(c, "losses_v2");
}

// swa = (swa * cnt + w) / (cnt + 1), each operation rounded on its own as numpy evaluates swa.py:29-31 on float32 arrays
__global__ __launch_bounds__(256) void swa_kernel(float* __restrict__ swa, const float* __restrict__ w, int64_t n, float cnt) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float a = swa[i] * cnt;
    const float b = a + w[i];
    swa[i] = b / (cnt + 1.f);
}

extern "C" {

int seld_k_losses_v2(const float* sed, const float* doa, const float* y_sed, const float* y_doa, const seld_v2_cfg* cfg, float* sloss, float* dloss,
                     float* dsed_pre, float* ddoa_pre, int B, int S, int nc) {
    if (!sed || !doa || !y_sed || !y_doa || !cfg || !sloss || !dloss || B < 1 || S < 1 || !v2_cfg_ok(cfg, nc)) return SELD_ERR_INVALID;
    const int rows = B * S;
    float* scr = nullptr;
    if (hipMalloc(&scr, ((size_t)loss_scratch_floats(rows) + 4) * sizeof(float) + 256) != hipSuccess) return SELD_ERR_NOMEM;
    float* den = scr + loss_scratch_floats(rows);
    launch_losses_v2(0, sed, doa, y_sed, y_doa, cfg, den, sloss, dloss, dsed_pre, ddoa_pre, scr, rows, nc, 0, 0);
    const bool ok = hipDeviceSynchronize() == hipSuccess && hipGetLastError() == hipSuccess;
    hipFree(scr);
    return ok ? SELD_OK : SELD_ERR_HIP;
}

int seld_k_reg_agc_adabelief(float* theta, float* g, float* m, float* v, int64_t n, int n_vars, const int64_t* off, const int32_t* rows,
                             const int32_t* cols, const int32_t* reg, float lr, float beta1, float beta2, float eps, float l2, float clip_factor,
                             int64_t step) {
    if (!theta || !g || !m || !v || !off || !rows || !cols || !reg || n <= 0 || n_vars < 1 || step < 1 || !(l2 >= 0.f)) return SELD_ERR_INVALID;
    V2Host H;
    if (!v2_build(n_vars, off, rows, cols, n, H)) return SELD_ERR_INVALID;
    const size_t bt = H.tiles.size() * sizeof(V2Tile), bs = H.segs.size() * sizeof(V2Seg), br = (size_t)n_vars * sizeof(int32_t);
    const size_t o1 = (bt + 255) & ~(size_t)255, o2 = o1 + ((bs + 255) & ~(size_t)255), o3 = o2 + ((br + 255) & ~(size_t)255);
    char* buf = nullptr;
    if (hipMalloc(&buf, o3 + (size_t)H.nunits * sizeof(float) + 256) != hipSuccess) return SELD_ERR_NOMEM;
    bool ok = hipMemcpy(buf, H.tiles.data(), bt, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(buf + o1, H.segs.data(), bs, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(buf + o2, reg, br, hipMemcpyHostToDevice) == hipSuccess;
    if (ok) {
        launch_v2_opt(0, theta, g, m, v, reinterpret_cast<const V2Tile*>(buf), (int)H.tiles.size(), reinterpret_cast<const V2Seg*>(buf + o1),
                      (int)H.segs.size(), reinterpret_cast<const int32_t*>(buf + o2), reinterpret_cast<float*>(buf + o3),
                      (float)v2_lr_t(lr, beta1, beta2, step), beta1, beta2, eps, l2, clip_factor);
        ok = hipDeviceSynchronize() == hipSuccess && hipGetLastError() == hipSuccess;
    }
    hipFree(buf);
    return ok ? SELD_OK : SELD_ERR_HIP;
}

int seld_train_fwd_bwd_v2(seld_ctx* c, const float* x, const float* y_sed, const float* y_doa, const seld_v2_cfg* cfg, float* sed, float* doa,
                          float* sloss, float* dloss) {
    if (!c || !x || !y_sed || !y_doa || !cfg) return SELD_ERR_INVALID;
    if (c->arch.n_classes > SELD_V2_MAX_CLASSES) return fail(c, SELD_ERR_INVALID, "trainv2: n_classes exceeds SELD_V2_MAX_CLASSES");
    if (!v2_cfg_ok(cfg, c->arch.n_classes)) return fail(c, SELD_ERR_INVALID, "trainv2: unknown sed_loss, or label_smoothing outside [0, 1)");
    if (c->dp_comm) return fail(c, SELD_ERR_UNSUPPORTED, "trainv2: the weighted losses are not defined across data-parallel ranks");
    HIPCHK(c, hipSetDevice(c->device));
    int rc = forward_impl(c, x, sed, doa, 1, true);
    if (rc) return rc;
    rc = run_losses_v2(c, y_sed, y_doa, cfg, sloss, dloss);
    if (rc) return rc;
    return backward_impl(c, x);
}

int seld_set_regularized(seld_ctx* c, const int32_t* flags, int n) {
    if (!c || !flags) return SELD_ERR_INVALID;
    if (n != (int)c->tr.size()) return fail(c, SELD_ERR_INVALID, "seld_set_regularized: one flag per trainable variable");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<int32_t> f(n);
    for (int i = 0; i < n; ++i) f[i] = flags[i] != 0;
    HIPCHK(c, hipMemcpy(c->v2.reg, f.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));
    return SELD_OK;
}

int seld_v2_opt_step(seld_ctx* c, float lr, float beta1, float beta2, float eps, float l2, float clip_factor) {
    if (!c) return SELD_ERR_INVALID;
    if (!(l2 >= 0.f)) return fail(c, SELD_ERR_INVALID, "seld_v2_opt_step: l2 must be >= 0");
    HIPCHK(c, hipSetDevice(c->device));
    c->adam_step += 1;
    PROF2(c, "v2_opt");
    launch_v2_opt(c->stream, c->params, c->grads, c->adam_m, c->adam_v, reinterpret_cast<const V2Tile*>(c->v2.tiles), c->v2.ntiles,
                  reinterpret_cast<const V2Seg*>(c->v2.segs), c->v2.nsegs, c->v2.reg, c->v2.scale, (float)v2_lr_t(lr, beta1, beta2, c->adam_step),
                  beta1, beta2, eps, l2, clip_factor);
    return check_launch(c, "v2_opt");
}

int seld_swa_update(seld_ctx* c) {
    if (!c) return SELD_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->swa_w) {
        int rc;
        if ((rc = dalloc(c, &c->swa_w, (size_t)c->nparam)) || (rc = dalloc(c, &c->swa_s, (size_t)std::max<int64_t>(c->nstate, 1)))) return rc;
    }
    if (c->swa_cnt == 0) {      // swa.py:26-27: the first update copies
        HIPCHK(c, hipMemcpyAsync(c->swa_w, c->params, (size_t)c->nparam * 4, hipMemcpyDeviceToDevice, c->stream));
        if (c->nstate) HIPCHK(c, hipMemcpyAsync(c->swa_s, c->state, (size_t)c->nstate * 4, hipMemcpyDeviceToDevice, c->stream));
    } else {
        hipLaunchKernelGGL(swa_kernel, dim3((unsigned)((c->nparam + 255) / 256)), dim3(256), 0, c->stream, c->swa_w, c->params, c->nparam, (float)c->swa_cnt);
        if (c->nstate)
            hipLaunchKernelGGL(swa_kernel, dim3((unsigned)((c->nstate + 255) / 256)), dim3(256), 0, c->stream, c->swa_s, c->state, c->nstate, (float)c->swa_cnt);
    }
    c->swa_cnt += 1;
    return check_launch(c, "swa_update");
}

int seld_swa_count(const seld_ctx* c) { return c ? c->swa_cnt : SELD_ERR_INVALID; }

int seld_swa_apply(seld_ctx* c) {
    if (!c) return SELD_ERR_INVALID;
    if (c->swa_cnt == 0) return fail(c, SELD_ERR_INVALID, "seld_swa_apply before the first seld_swa_update");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(c->params, c->swa_w, (size_t)c->nparam * 4, hipMemcpyDeviceToDevice, c->stream));
    if (c->nstate) HIPCHK(c, hipMemcpyAsync(c->state, c->swa_s, (size_t)c->nstate * 4, hipMemcpyDeviceToDevice, c->stream));
    return SELD_OK;
}

// ------------------------------------------------------------------------------------------------ the stream operators (composed models)
/* floats of caller scratch seld_v2_losses needs for `rows` = B * S label frames: the partials and the denominator slot behind them */
int64_t seld_v2_losses_scratch(int rows) { return rows > 0 ? (int64_t)loss_scratch_floats(rows) + 4 : -1; }

int seld_v2_losses(const float* sed, const float* doa, const float* y_sed, const float* y_doa, const seld_v2_cfg* cfg, float* sloss, float* dloss,
                     float* dsed_pre, float* ddoa_pre, float* scratch, int B, int S, int nc, void* stream) {
    if (!sed || !doa || !y_sed || !y_doa || !cfg || !sloss || !dloss || !scratch || B < 1 || S < 1 || !v2_cfg_ok(cfg, nc)) return SELD_ERR_INVALID;
    if ((uintptr_t)scratch & 7) return SELD_ERR_INVALID;      // the partials are doubles
    const int rows = B * S;
    launch_losses_v2((hipStream_t)stream, sed, doa, y_sed, y_doa, cfg, scratch + loss_scratch_floats(rows), sloss, dloss, dsed_pre, ddoa_pre, scratch,
                     rows, nc, 0, 0);
    return hipGetLastError() == hipSuccess ? SELD_OK : SELD_ERR_HIP;
}

namespace {
// v2_build's tables, the flags and the scale array in one device allocation
struct V2Plan { char* buf; const V2Tile* tiles; const V2Seg* segs; const int32_t* reg; float* scale; int ntiles, nsegs; };
}  // namespace

int seld_v2_plan_create(int64_t n, int n_vars, const int64_t* off, const int32_t* rows, const int32_t* cols, const int32_t* reg, void** plan) {
    if (!plan) return SELD_ERR_INVALID;
    *plan = nullptr;
    if (!off || !rows || !cols || !reg || n <= 0 || n_vars < 1) return SELD_ERR_INVALID;
    V2Host H;
    if (!v2_build(n_vars, off, rows, cols, n, H)) return SELD_ERR_INVALID;
    std::vector<int32_t> f(n_vars);
    for (int i = 0; i < n_vars; ++i) f[i] = reg[i] != 0;
    const size_t bt = H.tiles.size() * sizeof(V2Tile), bs = H.segs.size() * sizeof(V2Seg), br = (size_t)n_vars * sizeof(int32_t);
    const size_t o1 = (bt + 255) & ~(size_t)255, o2 = o1 + ((bs + 255) & ~(size_t)255), o3 = o2 + ((br + 255) & ~(size_t)255);
    char* buf = nullptr;
    if (hipMalloc(&buf, o3 + (size_t)H.nunits * sizeof(float) + 256) != hipSuccess) return SELD_ERR_NOMEM;
    if (hipMemcpy(buf, H.tiles.data(), bt, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(buf + o1, H.segs.data(), bs, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(buf + o2, f.data(), br, hipMemcpyHostToDevice) != hipSuccess) {
        hipFree(buf);
        return SELD_ERR_HIP;
    }
    *plan = new V2Plan{buf, reinterpret_cast<const V2Tile*>(buf), reinterpret_cast<const V2Seg*>(buf + o1), reinterpret_cast<const int32_t*>(buf + o2),
                       reinterpret_cast<float*>(buf + o3), (int)H.tiles.size(), (int)H.segs.size()};
    return SELD_OK;
}

void seld_v2_plan_destroy(void* plan) {
    V2Plan* p = static_cast<V2Plan*>(plan);
    if (!p) return;
    hipFree(p->buf);
    delete p;
}

int seld_v2_opt(void* plan, float* theta, float* g, float* m, float* v, float lr, float beta1, float beta2, float eps, float l2, float clip_factor,
                  int64_t step, void* stream) {
    const V2Plan* p = static_cast<const V2Plan*>(plan);
    if (!p || !theta || !g || !m || !v || step < 1 || !(l2 >= 0.f)) return SELD_ERR_INVALID;
    launch_v2_opt((hipStream_t)stream, theta, g, m, v, p->tiles, p->ntiles, p->segs, p->nsegs, p->reg, p->scale, (float)v2_lr_t(lr, beta1, beta2, step),
                  beta1, beta2, eps, l2, clip_factor);
    return hipGetLastError() == hipSuccess ? SELD_OK : SELD_ERR_HIP;
}

int seld_v2_swa(float* swa, const float* w, int64_t n, int cnt, void* stream) {
    if (!swa || !w || n <= 0 || cnt < 0) return SELD_ERR_INVALID;
    if (n > (int64_t)0x7fffffff * 256) return SELD_ERR_UNSUPPORTED;
    if (cnt == 0) {      // swa.py:26-27: the first update copies
        if (hipMemcpyAsync(swa, w, (size_t)n * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess) return SELD_ERR_HIP;
        return SELD_OK;
    }
    hipLaunchKernelGGL(swa_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, swa, w, n, (float)cnt);
    return hipGetLastError() == hipSuccess ? SELD_OK : SELD_ERR_HIP;
}

}  // extern "C"
