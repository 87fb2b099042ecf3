// kernels_api.hip — per-kernel C ABI entry points (include/seld_hip.h, "seld_k_*"): each runs ONE
// kernel family of the hot path on caller-provided device buffers so the parity tests can compare it
// with the oracle in isolation.  Null stream; scratch is allocated and freed per call (test use only).
#include "common.h"
#include <algorithm>
#include "../../include/seld_hip.h"
#include <vector>
#include <math.h>
#include <string.h>

namespace {
// the only process-wide choices of the library, all written by seld_k_set_option alone: what the seld_k_* entry points hand to the launchers, and
// four switches between kernel families that only these entry points have (a context has its own of each)
KernelChoices k_kc;
int k_conv64_split_bf16 = 1;
int k_conv1_split_bf16 = 1;
int k_rn_split_bf16 = 1;
int k_gemm_tn_split_bf16 = 1;
struct Scratch {
    std::vector<void*> p;
    float* get(size_t n) { void* q = nullptr; if (hipMalloc(&q, n * sizeof(float) + 256) != hipSuccess) return nullptr; p.push_back(q); return (float*)q; }
    ~Scratch() { hipDeviceSynchronize(); for (void* q : p) hipFree(q); }
};
int done() { return hipDeviceSynchronize() == hipSuccess && hipGetLastError() == hipSuccess ? SELD_OK : SELD_ERR_HIP; }

__global__ void coeffs_kernel(const float* mean, const float* invstd, const float* gamma, const float* beta, float* scale,
                              float* shift, int C) {
    const int c = threadIdx.x;
    if (c >= C) return;
    const float sc = gamma[c] * invstd[c];
    scale[c] = sc;
    shift[c] = beta[c] - mean[c] * sc;
}
}  // namespace

extern "C" {

int seld_k_set_option(const char* key, int value) {
    if (!key) return SELD_ERR_INVALID;
    if (!strcmp(key, "conv64_split_bf16")) { k_conv64_split_bf16 = value != 0; return SELD_OK; }
    if (!strcmp(key, "conv1_split_bf16")) { k_conv1_split_bf16 = value != 0; return SELD_OK; }
    if (!strcmp(key, "gemm_tn_split_bf16")) { k_gemm_tn_split_bf16 = value != 0; return SELD_OK; }
    if (!strcmp(key, "bf16_single")) { k_kc.mfma_one = value != 0; return SELD_OK; }
    if (!strcmp(key, "conv1_pingpong")) { k_kc.conv1_pingpong = value != 0; return SELD_OK; }
    if (!strcmp(key, "gsb_dbg")) { k_kc.gsb_dbg = value; return SELD_OK; }
    if (!strcmp(key, "xc_w16")) { k_kc.xc_w16 = value != 0; return SELD_OK; }
    if (!strcmp(key, "xc_xcd_map")) { k_kc.xc_xcd_map = value != 0; return SELD_OK; }
    if (!strcmp(key, "bwd_four_products")) { k_kc.bwd_four = value != 0; return SELD_OK; }
    if (!strcmp(key, "rn_split_bf16")) { k_rn_split_bf16 = value != 0; return SELD_OK; }
    if (!strcmp(key, "dgrad_r8")) { k_kc.dgrad_r8 = value != 0; return SELD_OK; }
    return SELD_ERR_INVALID;
}

int seld_k_conv3x3_fwd(const float* x, const float* w, const float* bias, float* z, float* stats, int B, int H, int W,
                       int Cin, int Cout) {
    if (!x || !w || !z || Cout != 64) return SELD_ERR_UNSUPPORTED;
    Scratch s;
    float* part = stats ? s.get((size_t)conv_stat_partial_capacity() * 128) : nullptr;
    if (stats && !part) return SELD_ERR_NOMEM;
    int np = 0, rc;
    if (Cin == 64 && k_conv64_split_bf16) {
        unsigned short* wsp = reinterpret_cast<unsigned short*>(s.get(9 * 3 * 4096 / 2 + 16));
        if (!wsp) return SELD_ERR_NOMEM;
        const float* ws[1] = {w}; unsigned short* ds[1] = {wsp}; const int fl[1] = {0};
        launch_split_weights_batch(0, k_kc, 1, ws, ds, fl);
        rc = launch_conv64_fwd_sb(0, k_kc, x, wsp, bias, z, part, &np, B, H, W);
    } else if (Cin == 64) rc = launch_conv64_fwd(0, x, w, bias, z, part, &np, B, H, W);
    else if (W == 64) rc = launch_conv_first_fwd(0, x, w, bias, z, part, &np, B, H, Cin);
    else return SELD_ERR_UNSUPPORTED;
    if (rc) return SELD_ERR_UNSUPPORTED;
    if (stats) launch_reduce_slabs(0, part, np, 128, stats, 128, 0);
    return done();
}

int seld_k_conv3x3_fwd_pre(const float* x, const float* pre_scale, const float* pre_shift, const float* w, const float* bias, float* z, float* stats,
                           float* pre_out, const float* ext_gamma, float* ext_out, int B, int H, int W) {
    if (!x || !w || !z || B <= 0 || H <= 0) return SELD_ERR_UNSUPPORTED;
    Scratch s;
    float* part = stats ? s.get((size_t)conv_stat_partial_capacity() * 128) : nullptr;
    if (stats && !part) return SELD_ERR_NOMEM;
    unsigned short* wsp = reinterpret_cast<unsigned short*>(s.get(9 * 3 * 4096 / 2 + 16));
    if (!wsp) return SELD_ERR_NOMEM;
    int np = 0;
    const float* ws[1] = {w}; unsigned short* ds[1] = {wsp}; const int fl[1] = {0};
    launch_split_weights_batch(0, k_kc, 1, ws, ds, fl);
    if (launch_conv64_fwd_sb(0, k_kc, x, wsp, bias, z, part, &np, B, H, W, pre_scale, pre_shift, pre_out, ext_gamma, ext_out)) return SELD_ERR_UNSUPPORTED;
    if (stats) launch_reduce_slabs(0, part, np, 128, stats, 128, 0);
    return done();
}

int seld_k_conv_first_fwd_pool(const float* x, const float* w, const float* bias, const float* gamma, float* z, float* zext,
                               unsigned char* amax, float* stats, int B, int H, int Cin) {
    if (!x || !w || !gamma || !zext || (z != nullptr && amax == nullptr)) return SELD_ERR_INVALID;
    Scratch s;
    float* part = stats ? s.get((size_t)conv_pool_stat_capacity() * 128) : nullptr;
    if (stats && !part) return SELD_ERR_NOMEM;
    int np = 0;
    if (launch_conv_first_fwd_pool(0, k_kc, x, w, bias, gamma, z, zext, amax, part, &np, B, H, Cin, k_conv1_split_bf16)) return SELD_ERR_UNSUPPORTED;
    if (stats) launch_reduce_slabs(0, part, np, 128, stats, 128, 0);
    return done();
}

int seld_k_bn_relu_ext(const float* zext, const float* scale, const float* shift, float* p, int64_t n) {
    if (!zext || !scale || !shift || !p) return SELD_ERR_INVALID;
    if (launch_bn_relu_ext(0, zext, scale, shift, p, n)) return SELD_ERR_UNSUPPORTED;
    return done();
}

int seld_k_conv3x3_dgrad(const float* dz, const float* w, float* dx, int B, int H, int W, int Cin, int Cout) {
    if (!dz || !w || !dx || Cin != 64 || Cout != 64) return SELD_ERR_UNSUPPORTED;
    Scratch s;
    float* wt = s.get(9 * 4096);
    if (!wt) return SELD_ERR_NOMEM;
    launch_flip_weights(0, w, wt);
    if (k_conv64_split_bf16) {
        unsigned short* wsp = reinterpret_cast<unsigned short*>(s.get(9 * 3 * 4096 / 2 + 16));
        if (!wsp) return SELD_ERR_NOMEM;
        // the model's own route: the flipped planes straight from w (prep.h split_weights_body, flip = 1) and the input-gradient launcher, which takes
        // the four-product form under option "bwd_four_products"
        const float* ws[1] = {w}; unsigned short* ds[1] = {wsp}; const int fl[1] = {1};
        launch_split_weights_batch(0, k_kc, 1, ws, ds, fl);
        launch_conv64_dgrad_sb(0, k_kc, dz, wsp, dx, B, H, W);
    } else
        launch_conv64_fwd(0, dz, wt, nullptr, dx, nullptr, nullptr, B, H, W);
    return done();
}

int seld_k_conv3x3_wgrad(const float* x, const float* dz, float* dw, float* db, int B, int H, int W, int Cin, int Cout) {
    if (!x || !dz || !dw || !db || Cout != 64) return SELD_ERR_UNSUPPORTED;
    Scratch s;
    float* slab = s.get((size_t)conv_wgrad_slab_capacity() * (9 * 4096 + 64));
    float* tmp = s.get(9 * 4096 + 64);
    if (!slab || !tmp) return SELD_ERR_NOMEM;
    int ns = 0;
    if (Cin == 64) {
        if (k_conv64_split_bf16 && conv64_wgrad_sb_usable(W)) {
            if (launch_conv64_wgrad_sb(0, k_kc, x, dz, slab, &ns, B, H, W)) return SELD_ERR_UNSUPPORTED;
        } else if (launch_conv64_wgrad(0, x, dz, slab, &ns, B, H, W)) return SELD_ERR_UNSUPPORTED;
        launch_reduce_slabs(0, slab, ns, 9 * 4096 + 64, tmp, 9 * 4096 + 64, 0);
        hipMemcpyAsync(dw, tmp, 9 * 4096 * 4, hipMemcpyDeviceToDevice, 0);
        hipMemcpyAsync(db, tmp + 9 * 4096, 64 * 4, hipMemcpyDeviceToDevice, 0);
    } else if (W == 64) {
        if (launch_conv_first_wgrad(0, x, dz, slab, &ns, B, H, Cin)) return SELD_ERR_UNSUPPORTED;
        launch_reduce_slabs(0, slab, ns, conv_first_wgrad_slab_stride(Cin), tmp, (int64_t)(9 * Cin + 1) * 64, 0);
        hipMemcpyAsync(dw, tmp, (size_t)9 * Cin * 64 * 4, hipMemcpyDeviceToDevice, 0);
        hipMemcpyAsync(db, tmp + 9 * Cin * 64, 64 * 4, hipMemcpyDeviceToDevice, 0);
    } else return SELD_ERR_UNSUPPORTED;
    return done();
}

int seld_k_conv1_bwd_fused(const float* x, const float* z, const float* dp, const float* mean, const float* invstd,
                           const float* gamma, const float* beta, float* dw, float* db, float* dgamma, float* dbeta,
                           int B, int H, int Cin, int pt, int pf) {
    if (!x || !z || !dp || !mean || !invstd || !gamma || !beta || !dw || !db || !dgamma || !dbeta) return SELD_ERR_INVALID;
    const int W = 64, C = 64;
    if (H % pt || W % pf) return SELD_ERR_UNSUPPORTED;
    Scratch s;
    float* coef = s.get(64 * 6);   // mean | invstd | scale | shift | c1 | c2
    float* part = s.get((size_t)bn_partial_capacity() * 128);
    float* pbuf = s.get((size_t)B * (H / pt) * (W / pf) * 64);
    float* slab = s.get((size_t)conv_wgrad_slab_capacity() * conv_first_wgrad_slab_stride(Cin));
    float* tmp = s.get(conv_first_wgrad_slab_stride(Cin));
    unsigned char* amax = reinterpret_cast<unsigned char*>(s.get(((size_t)B * (H / pt) * (W / pf) * 64 + 3) / 4));
    if (!coef || !part || !pbuf || !slab || !tmp || !amax) return SELD_ERR_NOMEM;
    hipMemcpyAsync(coef, mean, 256, hipMemcpyDeviceToDevice, 0);
    hipMemcpyAsync(coef + 64, invstd, 256, hipMemcpyDeviceToDevice, 0);
    hipLaunchKernelGGL(coeffs_kernel, dim3(1), dim3(64), 0, 0, mean, invstd, gamma, beta, coef + 128, coef + 192, C);
    if (launch_bn_relu_pool_fwd(0, z, coef + 128, coef + 192, pbuf, B, H, W, C, pt, pf)) return SELD_ERR_UNSUPPORTED;
    int np = 0, ns = 0;
    if (launch_bn_pool_bwd_reduce(0, z, pbuf, dp, coef, coef + 64, coef + 128, coef + 192, part, &np, B, H, W, C, pt, pf)) return SELD_ERR_UNSUPPORTED;
    launch_bn_bwd_finalize(0, part, np, (double)B * H * W, dgamma, dbeta, coef + 256, C);
    if (launch_pool_argext(0, z, gamma, amax, B, H, W, pt, pf)) return SELD_ERR_UNSUPPORTED;
    if (launch_conv_first_wgrad_fused(0, x, z, pbuf, dp, amax, coef, slab, &ns, B, H, Cin, pt, pf)) return SELD_ERR_UNSUPPORTED;
    launch_reduce_slabs(0, slab, ns, conv_first_wgrad_slab_stride(Cin), tmp, (int64_t)(9 * Cin + 1) * 64, 0);
    hipMemcpyAsync(dw, tmp, (size_t)9 * Cin * 64 * 4, hipMemcpyDeviceToDevice, 0);
    hipMemcpyAsync(db, tmp + 9 * Cin * 64, 64 * 4, hipMemcpyDeviceToDevice, 0);
    return done();
}

int seld_k_conv1_gram(const float* x, float* G, int B, int H, int Cin) {
    if (!x || !G) return SELD_ERR_INVALID;
    if (Cin != 7 && Cin != 10) return SELD_ERR_UNSUPPORTED;
    const size_t kp = (size_t)conv_gram_dim(Cin);
    Scratch s;
    float* slab = s.get((size_t)conv_gram_slab_capacity() * kp * kp);
    if (!slab) return SELD_ERR_NOMEM;
    int ns = 0;
    if (launch_conv_first_gram(0, k_kc, x, slab, &ns, B, H, Cin)) return SELD_ERR_UNSUPPORTED;
    launch_reduce_slabs(0, slab, ns, (int64_t)(kp * kp), G, (int64_t)(kp * kp), 0);
    return done();
}

int seld_k_conv1_train_gram(const float* x, const float* w, const float* bias, const float* gamma, const float* beta,
                            const float* dp, float* p, float* dw, float* db, float* dgamma, float* dbeta, int B, int H, int Cin) {
    if (!x || !w || !bias || !gamma || !beta || !dp || !p || !dw || !db || !dgamma || !dbeta) return SELD_ERR_INVALID;
    if ((Cin != 7 && Cin != 10) || H % 5) return SELD_ERR_UNSUPPORTED;
    const int W = 64, C = 64;
    const size_t np = (size_t)B * (H / 5) * 16 * 64, kp = (size_t)conv_gram_dim(Cin);
    Scratch s;
    float* coef = s.get(64 * 6);          // mean | invstd | scale | shift | c1 | c2
    float* mov = s.get(128);
    float* part = s.get((size_t)conv_pool_stat_capacity() * 128);
    float* bpart = s.get((size_t)bn_partial_capacity() * 128);
    float* zext = s.get(np);
    unsigned char* amax = reinterpret_cast<unsigned char*>(s.get((np + 3) / 4));
    float* gslab = s.get((size_t)conv_gram_slab_capacity() * kp * kp);
    float* gm = s.get(kp * kp);
    float* mslab = s.get((size_t)conv_msparse_slab_capacity() * kp * 64);
    float* mm = s.get(kp * 64);
    float* out = s.get((size_t)(9 * Cin + 1) * 64);
    if (!coef || !mov || !part || !bpart || !zext || !amax || !gslab || !gm || !mslab || !mm || !out) return SELD_ERR_NOMEM;
    hipMemsetAsync(mov, 0, 128 * sizeof(float), 0);
    int npart = 0, nb = 0, ns = 0;
    // forward without z: window extremes + positions + statistics; then BN coefficients and the pooled activation
    if (launch_conv_first_fwd_pool(0, k_kc, x, w, bias, gamma, nullptr, zext, amax, part, &npart, B, H, Cin, k_conv1_split_bf16)) return SELD_ERR_UNSUPPORTED;
    launch_bn_finalize(0, part, npart, (double)B * H * W, gamma, beta, mov, mov + 64, coef, coef + 64, coef + 128, coef + 192, C, 1);
    launch_bn_relu_ext(0, zext, coef + 128, coef + 192, p, (int64_t)np);
    // backward: BN sums from the pooled tensors, then dW = ka (G W + g b) + g kb + M
    if (launch_bn_pool_bwd_reduce(0, zext, p, dp, coef, coef + 64, coef + 128, coef + 192, bpart, &nb, B, H, W, C, 5, 4, 1))
        return SELD_ERR_UNSUPPORTED;
    launch_bn_bwd_finalize(0, bpart, nb, (double)B * H * W, dgamma, dbeta, coef + 256, C);
    if (launch_conv_first_gram(0, k_kc, x, gslab, &ns, B, H, Cin)) return SELD_ERR_UNSUPPORTED;
    launch_reduce_slabs(0, gslab, ns, (int64_t)(kp * kp), gm, (int64_t)(kp * kp), 0);
    if (launch_conv_first_msparse(0, x, p, dp, amax, coef + 128, mslab, &ns, B, H, Cin)) return SELD_ERR_UNSUPPORTED;
    launch_reduce_slabs(0, mslab, ns, (int64_t)(kp * 64), mm, (int64_t)(kp * 64), 0);
    launch_conv_first_assemble(0, gm, mm, w, bias, coef, out, out + 9 * Cin * 64, Cin);
    hipMemcpyAsync(dw, out, (size_t)9 * Cin * 64 * 4, hipMemcpyDeviceToDevice, 0);
    hipMemcpyAsync(db, out + 9 * Cin * 64, 64 * 4, hipMemcpyDeviceToDevice, 0);
    return done();
}

int seld_k_bn_relu_pool_fwd(const float* z, const float* scale, const float* shift, float* p, int B, int H, int W, int C,
                            int pt, int pf) {
    if (!z || !scale || !shift || !p) return SELD_ERR_INVALID;
    if (launch_bn_relu_pool_fwd(0, z, scale, shift, p, B, H, W, C, pt, pf)) return SELD_ERR_UNSUPPORTED;
    return done();
}

int seld_k_bn_relu_pool_bwd(const float* z, const float* dp, const float* mean, const float* invstd, const float* gamma,
                            const float* beta, float* dz, float* dgamma, float* dbeta, int B, int H, int W, int C, int pt,
                            int pf) {
    if (!z || !dp || !mean || !invstd || !gamma || !beta || !dz || !dgamma || !dbeta) return SELD_ERR_INVALID;
    if (C != 64) return SELD_ERR_UNSUPPORTED;
    Scratch s;
    float* coef = s.get(64 * 4);
    float* part = s.get((size_t)bn_partial_capacity() * 128);
    float* pbuf = s.get((size_t)B * (H / pt) * (W / pf) * 64);
    if (!coef || !part || !pbuf) return SELD_ERR_NOMEM;
    float *scale = coef, *shift = coef + 64, *c1c2 = coef + 128;
    hipLaunchKernelGGL(coeffs_kernel, dim3(1), dim3(64), 0, 0, mean, invstd, gamma, beta, scale, shift, C);
    int np = 0;
    if (launch_bn_relu_pool_fwd(0, z, scale, shift, pbuf, B, H, W, C, pt, pf)) return SELD_ERR_UNSUPPORTED;
    if (launch_bn_pool_bwd_reduce(0, z, pbuf, dp, mean, invstd, scale, shift, part, &np, B, H, W, C, pt, pf)) return SELD_ERR_UNSUPPORTED;
    launch_bn_bwd_finalize(0, part, np, (double)B * H * W, dgamma, dbeta, c1c2, C);
    launch_bn_pool_bwd_dz(0, z, dp, mean, invstd, scale, shift, c1c2, dz, B, H, W, C, pt, pf);
    return done();
}

int seld_k_gemm(const float* A, const float* Bm, const float* bias, float* C, int M, int N, int K, int transb, int act,
                int accumulate) {
    if (!A || !Bm || !C) return SELD_ERR_INVALID;
    if (launch_gemm(0, A, K, Bm, transb ? K : N, bias, C, N, M, N, K, transb, act, accumulate)) return SELD_ERR_INVALID;
    return done();
}

int seld_k_gemm_pair_n(const float* A, const float* B0, const float* B1, const float* bias0, const float* bias1, float* C0,
                       float* C1, int M, int N, int K, int transb, int act) {
    if (!A || !B0 || !B1 || !C0 || !C1) return SELD_ERR_INVALID;
    if (launch_gemm_dual_n(0, A, K, B0, B1, transb ? K : N, bias0, bias1, C0, C1, N, M, N, K, transb, act)) return SELD_ERR_INVALID;
    return done();
}

int seld_k_gemm_pair_k(const float* A0, const float* A1, const float* B0, const float* B1, const float* bias, float* C, int M,
                       int N, int K, int transb, int act, int accumulate) {
    if (!A0 || !A1 || !B0 || !B1 || !C) return SELD_ERR_INVALID;
    if (launch_gemm_dual_k(0, A0, A1, K, B0, B1, transb ? K : N, bias, C, N, M, N, K, transb, act, accumulate))
        return SELD_ERR_INVALID;
    return done();
}

int seld_k_gemm_sb(const float* A0, const float* A1, const float* B0, const float* B1, const float* bias0, const float* bias1,
                   float* C0, float* C1, int M, int N, int K, int transb, int act, int mode) {
    if (!A0 || !B0 || !C0 || mode < 0 || mode > 2 || (mode && !B1) || (mode == 1 && !C1) || (mode == 2 && !A1)) return SELD_ERR_INVALID;
    if (M <= 0 || N <= 0 || K <= 0 || !gemm_sb_usable(A0, K, N, K) || (mode == 2 && !gemm_sb_usable(A1, K, N, K))) return SELD_ERR_INVALID;
    Scratch s;
    const size_t ne = gemm_sb_split_elems(K, N);
    unsigned short* sp = reinterpret_cast<unsigned short*>(s.get(ne));   // 2 operands x ne bf16 = ne floats
    if (!sp) return SELD_ERR_NOMEM;
    const float* src[2] = {B0, B1};
    unsigned short* dst[2] = {sp, sp + ne};
    const int ldb[2] = {transb ? K : N, transb ? K : N}, tb[2] = {transb, transb}, Ks[2] = {K, K}, Ns[2] = {N, N};
    if (launch_gemm_split_b(0, k_kc, mode ? 2 : 1, src, dst, ldb, tb, Ks, Ns)) return SELD_ERR_INVALID;
    if (launch_gemm_sb(0, k_kc, false, GemmEpi(), A0, A1, K, dst[0], dst[1], bias0, bias1, C0, C1, N, M, N, K, act, mode)) return SELD_ERR_INVALID;
    return done();
}

int seld_k_xc_dw_bwd(const float* dy, const float* k, const float* xin, const float* add, const float* aff, const float* bn_mean,
                     const float* bn_invstd, float* dx, float* dk, float* sums, int B, int H, int fused) {
    if (!dy || !k || !xin || !dx || !dk || B < 1 || H < 1) return SELD_ERR_INVALID;
    const bool want_sums = bn_mean != nullptr;
    if (want_sums && (!bn_invstd || !sums || !aff || add)) return SELD_ERR_INVALID;      // the sums belong to the BatchNormalization folded into the loads
    const int64_t npix = (int64_t)B * H * 16;
    Scratch s;
    int ns = 0, np = 0;
    if (fused) {
        const int nb = xc_dw_fused_slabs(B, H);
        float* slab = s.get((size_t)nb * 576);
        float* tmp = s.get((size_t)reduce_slabs_groups(nb) * 576);
        float* part = s.get((size_t)nb * 128);
        float* folded = s.get((size_t)xc_partial_capacity() * 128);
        if (!slab || !tmp || !part || !folded) return SELD_ERR_NOMEM;
        if (launch_dw3x3_bwd_fused(0, k_kc, dy, k, xin, add, dx, slab, &ns, B, H, 16, aff, bn_mean, bn_invstd, want_sums ? part : nullptr)) return SELD_ERR_UNSUPPORTED;
        launch_reduce_slabs_2stage(0, slab, ns, 576, dk, 576, tmp);
        if (want_sums) {
            launch_xc_fold_partials(0, part, ns, folded, &np);
            launch_reduce_slabs(0, folded, np, 128, sums, 128, 0);
        }
    } else {
        float* slab = s.get((size_t)xc_partial_capacity() * 576);
        float* part = s.get((size_t)xc_partial_capacity() * 128);
        if (!slab || !part) return SELD_ERR_NOMEM;
        launch_dw3x3_bwd_data(0, k_kc, dy, k, xin, add, dx, B, H, 16, aff);
        launch_dw3x3_bwd_w(0, xin, dy, slab, &ns, B, H, 16, aff);
        launch_reduce_slabs(0, slab, ns, 576, dk, 576, 0);
        if (want_sums) {
            launch_xc_bn_bwd_reduce(0, xin, dx, bn_mean, bn_invstd, part, &np, npix);
            launch_reduce_slabs(0, part, np, 128, sums, 128, 0);
        }
    }
    return done();
}

// ---- xception_block's other kernels, one family per entry point (xception.hip): the launchers and combines of forward_xception / backward_xception
int seld_k_xc_dw_fwd(const float* x, const float* k, const float* aff, float* y, int B, int H, int W) {
    if (!x || !k || !y || B < 1 || H < 1 || W < 1) return SELD_ERR_INVALID;
    if ((int64_t)B * H * W > INT32_MAX) return SELD_ERR_UNSUPPORTED;      // the launcher's row count is an int
    if (launch_dw3x3_fwd(0, k_kc, x, k, y, B, H, W, aff)) return SELD_ERR_UNSUPPORTED;
    return done();
}

int seld_k_xc_unit_fwd(const float* x, const float* kdw, const float* wpw, const float* aff, float* dwo, float* z, float* sums, int B, int H,
                       int fused) {
    if (!x || !kdw || !wpw || !dwo || !z || B < 1 || H < 1) return SELD_ERR_INVALID;
    const int64_t npix = (int64_t)B * H * 16;
    if (npix > INT32_MAX) return SELD_ERR_UNSUPPORTED;      // tile / row counts and the product's M are ints
    Scratch s;
    float* part = sums ? s.get((size_t)xc_partial_capacity() * 128) : nullptr;
    if (sums && !part) return SELD_ERR_NOMEM;
    int np = 0;
    if (fused) {
        if (launch_xc_unit_fwd(0, x, kdw, wpw, dwo, z, part, &np, B, H, 16, aff)) return SELD_ERR_UNSUPPORTED;
    } else {
        if (launch_dw3x3_fwd(0, k_kc, x, kdw, dwo, B, H, 16, aff)) return SELD_ERR_UNSUPPORTED;
        if (launch_gemm(0, dwo, 64, wpw, 64, nullptr, z, 64, (int)npix, 64, 64, 0, 0, 0)) return SELD_ERR_UNSUPPORTED;
        if (sums) launch_xc_bn_stats(0, z, part, &np, npix);
    }
    if (sums) launch_reduce_slabs(0, part, np, 128, sums, 128, 0);
    return done();
}

int seld_k_xc_pw_bwd(const float* z, const float* gy, const float* dwo, const float* wpw, const float* mean, const float* invstd,
                     const float* scale, const float* c1c2, float* f1, float* dw, int64_t npix, int mode) {
    if (!z || !gy || !dwo || !wpw || !mean || !invstd || !scale || !c1c2 || !f1 || !dw || npix < 1 || mode < 0 || mode > 2) return SELD_ERR_INVALID;
    if (mode == 0 && npix > INT32_MAX) return SELD_ERR_UNSUPPORTED;      // the two products' M is an int
    Scratch s;
    int ns = 0;
    if (mode) {
        float* slab = s.get((size_t)xc_pw_bwd_slabs() * 4096);
        float* tmp = s.get((size_t)reduce_slabs_groups(xc_pw_bwd_slabs()) * 4096);
        if (!slab || !tmp) return SELD_ERR_NOMEM;
        if (launch_xc_pw_bwd(0, z, gy, dwo, wpw, mean, invstd, scale, c1c2, f1, slab, &ns, npix)) return SELD_ERR_UNSUPPORTED;
        if (mode == 2) launch_reduce_slabs_2stage(0, slab, ns, 4096, dw, 4096, tmp);      // the xc_nowait path's combine
        else launch_reduce_slabs(0, slab, ns, 4096, dw, 4096, 0);
    } else {
        const int splits = 512;      // backward_xception's: many short splits, the slab is only 64 x 64 (+ 64)
        float* dz = s.get((size_t)npix * 64);
        float* slab = s.get((size_t)splits * (4096 + 64));
        if (!dz || !slab) return SELD_ERR_NOMEM;
        launch_xc_bn_bwd_dz(0, z, gy, mean, invstd, scale, c1c2, dz, npix);
        if (launch_gemm_tn(0, dwo, 64, dz, 64, slab, &ns, (int)npix, 64, 64, 0, 0, 0, splits)) return SELD_ERR_UNSUPPORTED;
        launch_reduce_slabs2(0, slab, ns, 64 * 64 + 64, dw, 64 * 64, nullptr, 0);
        if (launch_gemm(0, dz, 64, wpw, 64, nullptr, f1, 64, (int)npix, 64, 64, 1, 0, 0)) return SELD_ERR_UNSUPPORTED;
    }
    return done();
}

int seld_k_xc_bn_stats(const float* z, float* sums, int64_t npix) {
    if (!z || !sums || npix < 1) return SELD_ERR_INVALID;
    Scratch s;
    float* part = s.get((size_t)xc_partial_capacity() * 128);
    if (!part) return SELD_ERR_NOMEM;
    int np = 0;
    if (launch_xc_bn_stats(0, z, part, &np, npix)) return SELD_ERR_UNSUPPORTED;
    launch_reduce_slabs(0, part, np, 128, sums, 128, 0);
    return done();
}

int seld_k_xc_bn_apply(const float* z, const float* scale, const float* shift, const float* res, float* out, int64_t npix) {
    if (!z || !scale || !shift || !out || npix < 1) return SELD_ERR_INVALID;
    if (npix > ((int64_t)1 << 35)) return SELD_ERR_UNSUPPORTED;      // one workgroup per 16 pixels: the grid is 32-bit
    if (launch_xc_bn_apply(0, z, scale, shift, res, out, npix)) return SELD_ERR_UNSUPPORTED;
    return done();
}

int seld_k_xc_bn_bwd(const float* z, const float* dy, const float* mean, const float* invstd, const float* scale, float* dz, float* dgamma,
                     float* dbeta, float* c1c2, int64_t npix) {
    if (!z || !dy || !mean || !invstd || !scale || !dz || !dgamma || !dbeta || !c1c2 || npix < 1) return SELD_ERR_INVALID;
    if (npix > ((int64_t)1 << 35)) return SELD_ERR_UNSUPPORTED;      // one workgroup per 16 pixels: the grid is 32-bit
    Scratch s;
    float* part = s.get((size_t)xc_partial_capacity() * 128);
    if (!part) return SELD_ERR_NOMEM;
    int np = 0;
    if (launch_xc_bn_bwd_reduce(0, z, dy, mean, invstd, part, &np, npix)) return SELD_ERR_UNSUPPORTED;
    launch_bn_bwd_finalize(0, part, np, (double)npix, dgamma, dbeta, c1c2, 64);
    launch_xc_bn_bwd_dz(0, z, dy, mean, invstd, scale, c1c2, dz, npix);
    return done();
}

int seld_k_gemm_tn(const float* A, const float* Bm, float* C, float* colsum, int M, int K1, int N) {
    if (!A || !Bm || !C) return SELD_ERR_INVALID;
    Scratch s;
    float* slab = s.get((size_t)gemm_tn_max_splits() * ((size_t)K1 * N + N));
    if (!slab) return SELD_ERR_NOMEM;
    int ns = 0;
    if (k_gemm_tn_split_bf16 && gemm_tn_sb_usable(A, K1, Bm, N, K1, N)) {
        if (launch_gemm_tn_sb(0, k_kc, A, K1, Bm, N, slab, &ns, M, N, 0, 0, colsum ? 1 : 0)) return SELD_ERR_INVALID;
    } else if (launch_gemm_tn(0, A, K1, Bm, N, slab, &ns, M, K1, N, 0, 0, colsum ? 1 : 0)) return SELD_ERR_INVALID;
    if (colsum) launch_reduce_slabs2(0, slab, ns, (int64_t)K1 * N + N, C, (int64_t)K1 * N, colsum, N);
    else launch_reduce_slabs(0, slab, ns, (int64_t)K1 * N + N, C, (int64_t)K1 * N, 0);
    return done();
}

int seld_k_gru_fwd(const float* gx_f, const float* gx_b, const float* U_f, const float* U_b, const float* brec_f,
                   const float* brec_b, float* h_f, float* h_b, float* saved_f, float* saved_b, float* out, int B, int S,
                   int units) {
    if (units != 128) return SELD_ERR_UNSUPPORTED;
    if (!gx_f || !gx_b || !U_f || !U_b || !brec_f || !brec_b || !h_f || !h_b) return SELD_ERR_INVALID;
    launch_gru_fwd(0, gx_f, gx_b, U_f, U_b, brec_f, brec_b, h_f, h_b, saved_f, saved_b, B, S);
    if (out) launch_mul(0, h_f, h_b, out, (int64_t)B * S * 128);
    return done();
}

int seld_k_gru_bwd(const float* dout, const float* h_f, const float* h_b, const float* saved_f, const float* saved_b,
                   const float* U_f, const float* U_b, float* dgx_f, float* dgx_b, float* dgh_f, float* dgh_b, int B, int S,
                   int units) {
    if (units != 128) return SELD_ERR_UNSUPPORTED;
    if (!dout || !h_f || !h_b || !saved_f || !saved_b || !U_f || !U_b || !dgx_f || !dgx_b || !dgh_f || !dgh_b) return SELD_ERR_INVALID;
    launch_gru_bwd(0, GRU_BWD_MUL, dout, nullptr, h_f, h_b, saved_f, saved_b, U_f, U_b, dgx_f, dgx_b, dgh_f, dgh_b, B, S);
    return done();
}

// the recurrent-dropout forms, as the training context launches them (forward.hip's forward_gru, backward.hip's backward_gru)
int seld_k_gru_drop_fwd(const float* gx_f, const float* gx_b, const float* U_f, const float* U_b, const float* brec_f, const float* brec_b,
                        const float* rm_f, const float* rm_b, float* h_f, float* h_b, float* hm_f, float* hm_b, float* saved_f, float* saved_b,
                        int B, int S, int units) {
    if (units != 128) return SELD_ERR_UNSUPPORTED;
    if (!gx_f || !gx_b || !U_f || !U_b || !brec_f || !brec_b || !rm_f || !rm_b || !h_f || !h_b || !hm_f || !hm_b || !saved_f || !saved_b || B < 1 ||
        S < 1)
        return SELD_ERR_INVALID;
    if (launch_gru_fwd(0, gx_f, gx_b, U_f, U_b, brec_f, brec_b, h_f, h_b, saved_f, saved_b, B, S, rm_f, rm_b, hm_f, hm_b)) return SELD_ERR_INVALID;
    return done();
}

int seld_k_gru_drop_bwd(const float* dout, const float* h_f, const float* h_b, const float* hm_f, const float* hm_b, const float* saved_f,
                        const float* saved_b, const float* U_f, const float* U_b, const float* rm_f, const float* rm_b, float* dgx_f, float* dgx_b,
                        float* dgh_f, float* dgh_b, int B, int S, int units) {
    if (units != 128) return SELD_ERR_UNSUPPORTED;
    if (!dout || !h_f || !h_b || !hm_f || !hm_b || !saved_f || !saved_b || !U_f || !U_b || !rm_f || !rm_b || !dgx_f || !dgx_b || !dgh_f || !dgh_b ||
        B < 1 || S < 1)
        return SELD_ERR_INVALID;
    if (launch_gru_bwd(0, GRU_BWD_MUL, dout, nullptr, h_f, h_b, saved_f, saved_b, U_f, U_b, dgx_f, dgx_b, dgh_f, dgh_b, B, S, rm_f, rm_b, hm_f, hm_b))
        return SELD_ERR_INVALID;
    return done();
}

int seld_k_losses(const float* sed, const float* doa, const float* y_sed, const float* y_doa, const seld_loss_cfg* cfg,
                  float* sloss, float* dloss, float* dsed_pre, float* ddoa_pre, int B, int S, int nc) {
    if (!sed || !doa || !y_sed || !y_doa || !cfg || !sloss || !dloss) return SELD_ERR_INVALID;
    Scratch s;
    const int rows = B * S;
    float* scr = s.get((size_t)loss_scratch_floats(rows));
    float* den = s.get(4);
    if (!scr || !den) return SELD_ERR_NOMEM;
    if (cfg->doa_loss == SELD_DOA_MMSE) {
        if (cfg->mmse_den > 0.f) hipMemcpy(den, &cfg->mmse_den, 4, hipMemcpyHostToDevice);
        else launch_mmse_den(0, y_doa, den, scr, rows, nc);
    }
    launch_losses(0, sed, doa, y_sed, y_doa, cfg->doa_loss, cfg->w_sed, cfg->w_doa, cfg->sed_grad_scale, den, sloss, dloss,
                  dsed_pre, ddoa_pre, scr, B, S, nc);
    return done();
}

int seld_k_adam(float* theta, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                int64_t step) {
    if (!theta || !g || !m || !v || n <= 0 || step < 1) return SELD_ERR_INVALID;
    const double t = (double)step;
    const float lr_t = (float)((double)lr * sqrt(1.0 - pow((double)beta2, t)) / (1.0 - pow((double)beta1, t)));
    launch_adam(0, theta, g, m, v, n, lr_t, beta1, beta2, eps);
    return done();
}

// ---- loss_adam.hip's other kernels and launcher arguments, one launcher per entry point: what api.hip's run_losses / seld_adam_step, forward.hip's
// forward_heads / forward_gru and backward.hip's backward_heads / backward_gru pass.  Every refusal comes before the first HIP call.
static bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static bool loss_args_ok(const seld_loss_cfg* cfg, const float* scratch, int B, int S, int nc) {
    return cfg && scratch && ((uintptr_t)scratch & 7) == 0 && B >= 1 && S >= 1 && nc >= 1 && (int64_t)B * S <= INT32_MAX / 4 &&
           cfg->doa_loss >= SELD_DOA_MSE && cfg->doa_loss <= SELD_DOA_MSLE;
}

int seld_k_losses_strided(const float* sed, const float* doa, const float* y_sed, const float* y_doa, const seld_loss_cfg* cfg, float* sloss,
                          float* dloss, float* dsed_pre, int ld_sed, float* ddoa_pre, int ld_doa, float* scratch, int B, int S, int nc,
                          int defer_finalize) {
    if (!sed || !doa || !y_sed || !y_doa || !sloss || !dloss || !loss_args_ok(cfg, scratch, B, S, nc)) return SELD_ERR_INVALID;
    if ((ld_sed > 0 && ld_sed < nc) || (ld_doa > 0 && ld_doa < 3 * nc)) return SELD_ERR_INVALID;      // <= 0: dense rows, as the launcher reads it
    const int rows = B * S;
    float* den = scratch + loss_scratch_floats(rows);
    if (cfg->doa_loss == SELD_DOA_MMSE) {
        if (cfg->mmse_den > 0.f) launch_fill(0, den, 1, cfg->mmse_den);
        else launch_mmse_den(0, y_doa, den, scratch, rows, nc);
    }
    launch_losses(0, sed, doa, y_sed, y_doa, cfg->doa_loss, cfg->w_sed, cfg->w_doa, cfg->sed_grad_scale, den, sloss, dloss, dsed_pre, ddoa_pre, scratch,
                  B, S, nc, ld_sed, ld_doa, defer_finalize ? 1 : 0);
    return done();
}

int seld_k_losses_finalize(const seld_loss_cfg* cfg, float* sloss, float* dloss, float* scratch, int B, int S, int nc) {
    if (!sloss || !dloss || !loss_args_ok(cfg, scratch, B, S, nc)) return SELD_ERR_INVALID;
    launch_losses_finalize(0, cfg->doa_loss, scratch + loss_scratch_floats(B * S), sloss, dloss, scratch, B, S, nc);
    return done();
}

int seld_k_agc(const float* theta, float* g, int64_t off, int rank, const int64_t* shape) {
    if (!theta || !g || !shape || off < 0 || rank < 1 || rank > 4) return SELD_ERR_INVALID;
    int64_t n = 1;
    for (int i = 0; i < rank; ++i) {
        if (shape[i] < 1 || shape[i] > INT32_MAX || n * shape[i] > INT32_MAX) return SELD_ERR_INVALID;      // the launcher's rows and cols are ints
        n *= shape[i];
    }
    launch_agc(0, theta, g, off, rank, shape, nullptr);
    return done();
}

int seld_k_act_bwd(const float* y, float* dy, int64_t n, int act) {
    if (!y || !dy || n < 1 || (n & 3) || act < 1 || act > 3 || !al16(y) || !al16(dy)) return SELD_ERR_INVALID;
    if (launch_act_bwd(0, y, dy, n, act)) return SELD_ERR_INVALID;
    return done();
}

int seld_k_v1_couple_fwd(const float* sed, const float* doa1, float* out, float* out2, int rows, int nc) {
    if (!sed || !doa1 || !out || rows < 1 || nc < 1) return SELD_ERR_INVALID;
    launch_v1_couple_fwd(0, sed, doa1, out, out2, rows, nc);
    return done();
}

int seld_k_v1_couple_bwd(const float* sed, const float* doa1, float* dsed_pre, int ld_sed, float* ddoa_pre, int ld_doa, int rows, int nc) {
    if (!sed || !doa1 || !dsed_pre || !ddoa_pre || rows < 1 || nc < 1 || ld_sed < nc || ld_doa < 3 * nc) return SELD_ERR_INVALID;
    launch_v1_couple_bwd(0, sed, doa1, dsed_pre, ld_sed, ddoa_pre, ld_doa, rows, nc);
    return done();
}

int seld_k_time_expand(const float* x, float* xe, int B, int S, int C, int ks) {
    if (!x || !xe || B < 1 || S < 1 || C < 1 || ks < 1 || (C & 3) || !al16(x) || !al16(xe)) return SELD_ERR_INVALID;
    if (launch_time_expand(0, x, xe, B, S, C, ks)) return SELD_ERR_INVALID;
    return done();
}

int seld_k_time_fold(const float* dxe, float* dx, int B, int S, int C, int ks, int accumulate) {
    if (!dxe || !dx || B < 1 || S < 1 || C < 1 || ks < 1 || (C & 3) || !al16(dxe) || !al16(dx)) return SELD_ERR_INVALID;
    if (launch_time_fold(0, dxe, dx, B, S, C, ks, accumulate)) return SELD_ERR_INVALID;
    return done();
}

int seld_k_mask_rows(const float* in, const float* mask, float* out, int64_t rows, int S, int F, int accumulate) {
    if (!in || !mask || !out || rows < 1 || S < 1 || F < 1 || (F & 3) || !al16(in) || !al16(mask) || !al16(out)) return SELD_ERR_INVALID;
    if (launch_mask_rows(0, in, mask, out, rows, S, F, accumulate)) return SELD_ERR_INVALID;
    return done();
}

int seld_k_dropout4(const float* in, float* out, int64_t n, float rate, uint64_t seed, unsigned layer, unsigned step) {
    if (!in || !out || n < 1 || (n & 3) || !(rate >= 0.f && rate < 1.f) || !al16(in) || !al16(out)) return SELD_ERR_INVALID;
    if (launch_dropout(0, in, out, n, rate, seed, layer, step)) return SELD_ERR_INVALID;
    return done();
}

// VALU-only load on `blocks` CUs (the recurrence's shape); lane 0 of every block reports shader cycles and 100 MHz ticks
__global__ __launch_bounds__(512) void valu_clock_kernel(unsigned long long* out, int iters, float seed) {
    float a = seed + threadIdx.x * 1e-9f, b = seed * 0.5f;
    const unsigned long long c0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    for (int i = 0; i < iters; ++i) {
        a = fmaf(a, 1.0000001f, 1e-9f);
        b = fmaf(b, 0.9999999f, 1e-9f);
    }
    const unsigned long long c1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    if (threadIdx.x == 0) {
        out[3 * blockIdx.x] = c1 - c0;
        out[3 * blockIdx.x + 1] = r1 - r0;
        out[3 * blockIdx.x + 2] = (unsigned long long)__float_as_uint(a + b);   // keeps the loop alive
    }
}

int seld_k_valu_clock_mhz(int blocks, double* mhz) {
    if (!mhz || blocks < 1 || blocks > 1024) return SELD_ERR_INVALID;
    unsigned long long* d = nullptr;
    if (hipMalloc(&d, (size_t)blocks * 3 * sizeof(unsigned long long)) != hipSuccess) return SELD_ERR_NOMEM;
    std::vector<unsigned long long> h((size_t)blocks * 3);
    for (int rep = 0; rep < 2; ++rep)      // the second launch is measured (clocks settled)
        hipLaunchKernelGGL(valu_clock_kernel, dim3(blocks), dim3(512), 0, 0, d, 200000, 1.0f);
    const bool ok = hipMemcpy(h.data(), d, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost) == hipSuccess;
    hipFree(d);
    if (!ok) return SELD_ERR_HIP;
    std::vector<double> r;
    for (int i = 0; i < blocks; ++i)
        if (h[3 * i + 1]) r.push_back(100.0 * (double)h[3 * i] / (double)h[3 * i + 1]);
    if (r.empty()) return SELD_ERR_HIP;
    std::sort(r.begin(), r.end());
    *mhz = r[r.size() / 2];
    return SELD_OK;
}

// ---- resnet50_block pieces (resnet.hip + the fp32 GEMMs), as api.hip composes them
// split `w` ([K,N]; transposed: the planes of w^T) into scratch planes when the split-bf16 product takes the shape, as the model does per step
// transposed == 2: the matrix of a 3x3 kernel's input-gradient convolution (K = 9 Cin: flipped taps, channels swapped)
static unsigned short* rn_k_split(Scratch& s, const float* w, int K, int N, int transposed) {
    if (!k_rn_split_bf16 || !(transposed ? rn_sb_dgrad_ok(K, N) : rn_sb_fwd_ok(K, N))) return nullptr;
    unsigned short* d = reinterpret_cast<unsigned short*>(s.get((gemm_sb_split_elems(K, N) + 1) / 2));
    if (!d) return nullptr;
    const float* src[1] = {w}; unsigned short* dst[1] = {d};
    const int ldb[1] = {N}, tb[1] = {transposed}, Ks[1] = {transposed == 2 ? 9 * N : transposed ? N : K}, Ns[1] = {transposed == 2 ? K / 9 : transposed ? K : N};
    return launch_gemm_split_b(0, k_kc, 1, src, dst, ldb, tb, Ks, Ns) ? nullptr : d;
}

// sums (optional, device, ceil(Cout / 64) * 128 + 1 doubles): the BatchNorm statistics from the product's epilogue as the model takes them (GemmEpi
// stat_part, a partial buffer of rn_epi_partial_floats), folded by rn_bn_finalize's phase 1: per 64-channel chunk [sum z | sum z^2], then M
int seld_k_rn_conv_stats(const float* x, const float* w, float* z, int B, int H, int W, int Cin, int Cout, int ksize, int stride_f, double* sums) {
    if (!x || !w || !z) return SELD_ERR_INVALID;
    if ((ksize != 1 && ksize != 3) || (ksize == 3 && stride_f != 1) || stride_f < 1 || W % stride_f || Cin % 4) return SELD_ERR_UNSUPPORTED;
    if (sums && Cout % 32) return SELD_ERR_UNSUPPORTED;
    const int Wo = W / stride_f;
    const int M = B * H * Wo, K = ksize * ksize * Cin;
    Scratch s;
    const unsigned short* wsp = rn_k_split(s, w, K, Cout, 0);
    const size_t cap = sums ? rn_epi_partial_floats(M, Cout) : 0;
    float* part = sums ? s.get(cap) : nullptr;
    if (sums && !part) return SELD_ERR_NOMEM;
    int nbx = 0;
    if (ksize == 1) {
        if (launch_rn_product_fwd(0, k_kc, x, Cin * stride_f, w, wsp, z, M, K, Cout, part, &nbx, cap)) return SELD_ERR_INVALID;
    } else if (wsp && rn_conv3_sb_ok(Cin, Cout)) {      // im2col rows formed on load
        if (launch_rn_conv3_fwd(0, k_kc, x, wsp, z, B, H, W, Cin, Cout, part, &nbx, cap)) return SELD_ERR_INVALID;
    } else {
        float* col = s.get((size_t)M * 9 * Cin);
        if (!col) return SELD_ERR_NOMEM;
        launch_im2col3x3(0, x, col, B, H, W, Cin);
        if (launch_rn_product_fwd(0, k_kc, col, K, w, wsp, z, M, K, Cout, part, &nbx, cap)) return SELD_ERR_INVALID;
    }
    // phase 1 folds the partials and stops: gamma, beta, the moving statistics and the coefficients are not touched
    if (sums) launch_rn_bn_finalize(0, part, nbx, (double)M, nullptr, nullptr, nullptr, nullptr, nullptr, Cout, 1, sums, 1);
    return done();
}
int seld_k_rn_conv(const float* x, const float* w, float* z, int B, int H, int W, int Cin, int Cout, int ksize, int stride_f) {
    return seld_k_rn_conv_stats(x, w, z, B, H, W, Cin, Cout, ksize, stride_f, nullptr);
}

// addg + gate4 (optional, ksize 1, stride_f 1): dx += addg [gate bit] as the model adds the identity shortcut's gradient — in the input-gradient
// product's epilogue where launch_rn_product_dgrad takes it, else by launch_rn_add_gated behind it
int seld_k_rn_conv_bwd_add(const float* x, const float* w, const float* dz, float* dw, float* dx, int B, int H, int W, int Cin, int Cout,
                           int ksize, int stride_f, const float* addg, const unsigned char* gate4) {
    if (!x || !w || !dz || !dw || !dx || (!addg != !gate4)) return SELD_ERR_INVALID;
    if ((ksize != 1 && ksize != 3) || (ksize == 3 && stride_f != 1) || stride_f < 1 || W % stride_f || Cin % 4) return SELD_ERR_UNSUPPORTED;
    if (addg && (ksize != 1 || stride_f != 1)) return SELD_ERR_UNSUPPORTED;
    const int Wo = W / stride_f, M = B * H * Wo, K1 = ksize * ksize * Cin;
    Scratch s;
    const int64_t cap = tn_slab_capacity();     // the model's slab buffer
    float* slab = s.get((size_t)cap);
    if (!slab) return SELD_ERR_NOMEM;
    if (ksize == 3 && k_rn_split_bf16 && rn_conv3_sb_ok(Cin, Cout)) {      // both gradients with the im2col rows formed on load
        const unsigned short* wsp_f = rn_k_split(s, w, K1, Cout, 2);
        if (!wsp_f) return SELD_ERR_NOMEM;
        if (launch_rn_conv3_wgrad(0, k_kc, x, dz, slab, cap, dw, B, H, W, Cin, Cout)) return SELD_ERR_INVALID;
        if (launch_rn_conv3_dgrad(0, k_kc, dz, wsp_f, dx, B, H, W, Cin, Cout)) return SELD_ERR_INVALID;
        return done();
    }
    float* col = ksize == 3 ? s.get((size_t)M * 9 * Cin) : nullptr;
    float* dcol = ksize == 3 ? s.get((size_t)M * 9 * Cin) : nullptr;
    if (ksize == 3 && (!col || !dcol)) return SELD_ERR_NOMEM;
    const unsigned short* wsp_t = rn_k_split(s, w, K1, Cout, 1);
    if (ksize == 3) {
        launch_im2col3x3(0, x, col, B, H, W, Cin);
        if (launch_rn_product_wgrad(0, k_kc, col, K1, dz, slab, cap, dw, M, K1, Cout, k_rn_split_bf16)) return SELD_ERR_INVALID;
        if (launch_rn_product_dgrad(0, k_kc, dz, w, wsp_t, dcol, K1, M, K1, Cout, 0)) return SELD_ERR_INVALID;
        launch_col2im3x3(0, dcol, dx, B, H, W, Cin);
    } else {
        const int ldx = Cin * stride_f;
        if (launch_rn_product_wgrad(0, k_kc, x, ldx, dz, slab, cap, dw, M, K1, Cout, k_rn_split_bf16)) return SELD_ERR_INVALID;
        if (stride_f > 1 && hipMemsetAsync(dx, 0, (size_t)B * H * W * Cin * sizeof(float), 0) != hipSuccess) return SELD_ERR_HIP;
        const int added = launch_rn_product_dgrad(0, k_kc, dz, w, wsp_t, dx, ldx, M, K1, Cout, 0, addg, gate4);
        if (added < 0) return SELD_ERR_INVALID;
        if (addg && added == 1) launch_rn_add_gated(0, dx, addg, gate4, (int64_t)M * Cin);
    }
    return done();
}
int seld_k_rn_conv_bwd(const float* x, const float* w, const float* dz, float* dw, float* dx, int B, int H, int W, int Cin, int Cout,
                       int ksize, int stride_f) {
    return seld_k_rn_conv_bwd_add(x, w, dz, dw, dx, B, H, W, Cin, Cout, ksize, stride_f, nullptr, nullptr);
}

int seld_k_rn_bn(const float* z, const float* gamma, const float* beta, const float* res, float* out, float* mean, float* invstd,
                 int64_t npix, int C, int relu) {
    if (!z || !gamma || !beta || !out) return SELD_ERR_INVALID;
    if (C % 32 || npix <= 0) return SELD_ERR_UNSUPPORTED;
    Scratch s;
    float* part = s.get((size_t)rn_partial_capacity() * ((C + 63) / 64) * 128);
    float* coef = s.get((size_t)6 * C);
    float* mov = s.get((size_t)2 * C);
    if (!part || !coef || !mov) return SELD_ERR_NOMEM;
    if (hipMemsetAsync(mov, 0, (size_t)2 * C * sizeof(float), 0) != hipSuccess) return SELD_ERR_HIP;
    int nbx = 0;
    if (launch_rn_bn_stats(0, z, part, &nbx, npix, C)) return SELD_ERR_UNSUPPORTED;
    launch_rn_bn_finalize(0, part, nbx, (double)npix, gamma, beta, mov, mov + C, coef, C, 1);
    launch_rn_bn_apply(0, z, coef, res, out, npix, C, relu);
    if (mean && hipMemcpyAsync(mean, coef, C * sizeof(float), hipMemcpyDeviceToDevice, 0) != hipSuccess) return SELD_ERR_HIP;
    if (invstd && hipMemcpyAsync(invstd, coef + C, C * sizeof(float), hipMemcpyDeviceToDevice, 0) != hipSuccess) return SELD_ERR_HIP;
    return done();
}

int seld_k_rn_bn_bwd(const float* z, const float* dy, const float* mask, const float* gamma, float* dz, float* dgamma, float* dbeta,
                     int64_t npix, int C) {
    if (!z || !dy || !gamma || !dz || !dgamma || !dbeta) return SELD_ERR_INVALID;
    if (C % 32 || npix <= 0) return SELD_ERR_UNSUPPORTED;
    Scratch s;
    float* part = s.get((size_t)rn_partial_capacity() * ((C + 63) / 64) * 128);
    float* coef = s.get((size_t)6 * C);
    float* mov = s.get((size_t)3 * C);
    if (!part || !coef || !mov) return SELD_ERR_NOMEM;
    if (hipMemsetAsync(mov, 0, (size_t)3 * C * sizeof(float), 0) != hipSuccess) return SELD_ERR_HIP;
    int nbx = 0;
    launch_rn_bn_stats(0, z, part, &nbx, npix, C);
    launch_rn_bn_finalize(0, part, nbx, (double)npix, gamma, mov + 2 * C, mov, mov + C, coef, C, 1);     // beta plays no part in the backward
    launch_rn_bn_bwd_reduce(0, z, dy, mask, coef, part, &nbx, npix, C);
    launch_rn_bn_bwd_finalize(0, part, nbx, (double)npix, dgamma, dbeta, coef, C);
    launch_rn_bn_bwd_dz(0, z, dy, mask, coef, dz, npix, C);
    return done();
}

// ---- the GEMM family's launchers with every argument the model passes (gemm.hip, gemm_sb.hip, gemm_tn_sb.hip, prep.hip): leading dimensions,
// modes, epilogues, split limits, jobs.  Pass-throughs: what a launcher refuses comes back as SELD_ERR_INVALID, before anything is written to an output.
int seld_k_gemm_ex(const float* A, int lda, const float* Bm, int ldb, const float* bias, float* C, int ldc, int M, int N, int K, int transb, int act,
                   int accumulate, int mode, const float* A1, const float* B1, const float* bias1, float* C1, float* M0, float* M1, int nsplit,
                   float* stat_part, const float* addg) {
    if (!A || !Bm || !C || mode < 0 || mode > 4) return SELD_ERR_INVALID;
    if ((mode == 1 && (!B1 || !C1)) || (mode == 2 && (!A1 || !B1)) || (mode == 3 && !C1)) return SELD_ERR_INVALID;
    if (mode == 4 && (!C1 || transb || nsplit < 1 || nsplit >= N || accumulate)) return SELD_ERR_INVALID;
    if (mode && (stat_part || addg)) return SELD_ERR_INVALID;
    GemmEpi epi;
    epi.stat_part = stat_part; epi.addg = addg;
    int rc;
    if (mode == 0) rc = launch_gemm(0, A, lda, Bm, ldb, bias, C, ldc, M, N, K, transb, act, accumulate, epi);
    else if (mode == 1) rc = launch_gemm_dual_n(0, A, lda, Bm, B1, ldb, bias, bias1, C, C1, ldc, M, N, K, transb, act);
    else if (mode == 2) rc = launch_gemm_dual_k(0, A, A1, lda, Bm, B1, ldb, bias, C, ldc, M, N, K, transb, act, accumulate);
    else if (mode == 3) rc = launch_gemm_mirror(0, A, lda, Bm, ldb, bias, C, C1, ldc, M, N, K, transb, act);
    else rc = launch_gemm_heads(0, A, lda, Bm, bias, C, C1, M0, M1, M, nsplit, N - nsplit, K, act & 15, act >> 4);
    if (rc) return SELD_ERR_INVALID;
    return done();
}

// B0 / B1 are split here as the model's callers do: transb 0 = [K][N] (a forward product), 1 = [N][K] and 2 = a 3x3 kernel [9][N][ldb] read as the
// matrix of its input-gradient convolution; a transposed job's mid plane is rounded, which is what the four-product form (`backward`) reads
int seld_k_gemm_sb_ex(const float* A0, const float* A1, int lda, const float* B0, const float* B1, int ldb, int transb, const float* bias0,
                      const float* bias1, float* C0, float* C1, int ldc, int M, int N, int K, int act, int mode, int accum, int backward,
                      float* stat_part, const float* addg, const unsigned char* gate4, int conv_C, int conv_H, int conv_W) {
    if (!A0 || !B0 || !C0 || mode < 0 || mode > 2 || (mode && !B1) || (mode == 1 && !C1) || (mode == 2 && !A1) || transb < 0 || transb > 2) return SELD_ERR_INVALID;
    if (M <= 0 || N <= 0 || K <= 0 || (K % 32) || (backward && !transb)) return SELD_ERR_INVALID;
    Scratch s;
    const size_t ne = gemm_sb_split_elems(K, N);
    unsigned short* sp = reinterpret_cast<unsigned short*>(s.get(ne));   // 2 operands x ne bf16 = ne floats
    if (!sp) return SELD_ERR_NOMEM;
    const float* src[2] = {B0, B1};
    unsigned short* dst[2] = {sp, sp + ne};
    const int ldbs[2] = {ldb, ldb}, tb[2] = {transb, transb}, Ks[2] = {K, K}, Ns[2] = {N, N};
    if (launch_gemm_split_b(0, k_kc, mode ? 2 : 1, src, dst, ldbs, tb, Ks, Ns)) return SELD_ERR_INVALID;
    GemmEpi epi;
    epi.stat_part = stat_part; epi.addg = addg; epi.gate4 = gate4;
    if (launch_gemm_sb(0, k_kc, backward != 0, epi, A0, A1, lda, dst[0], mode ? dst[1] : nullptr, bias0, bias1, C0, C1, ldc, M, N, K, act, mode, accum,
                       conv_C, conv_H, conv_W))
        return SELD_ERR_INVALID;
    return done();
}

int seld_k_gemm_tn_ex(const float* A, int lda, const float* Bm, int ldb, float* C, float* colsum, int M, int K1, int N, int S, int shift,
                      int want_bias, int max_splits, int chunk_rows, int* nslab) {
    if (!A || !Bm || !C || !nslab || (want_bias != 0) != (colsum != nullptr) || M <= 0 || K1 <= 0 || N <= 0 || max_splits < 0) return SELD_ERR_INVALID;
    Scratch s;
    const int64_t per = (int64_t)K1 * N + N;
    float* slab = s.get((size_t)(max_splits ? max_splits : gemm_tn_max_splits()) * per);
    if (!slab) return SELD_ERR_NOMEM;
    int ns = 0;
    if (launch_gemm_tn(0, A, lda, Bm, ldb, slab, &ns, M, K1, N, S, shift, want_bias, max_splits, chunk_rows)) return SELD_ERR_INVALID;
    if (colsum) launch_reduce_slabs2(0, slab, ns, per, C, (int64_t)K1 * N, colsum, N);
    else launch_reduce_slabs(0, slab, ns, per, C, (int64_t)K1 * N, 0);
    *nslab = ns;
    return done();
}

// 1 .. TN_MAX_JOBS products of one shape in one launch (K1 = 128), combined by the batch reduction; colsum (an array of njobs pointers) with want_bias
int seld_k_gemm_tn_sb_ex(int njobs, const float* const* A, const int* lda, const int* shift, const float* const* Bm, int ldb, float* const* C,
                         float* const* colsum, int M, int N, int S, int want_bias, int* nslab) {
    if (njobs < 1 || njobs > TN_MAX_JOBS || !A || !lda || !shift || !Bm || !C || !nslab || (want_bias != 0) != (colsum != nullptr) || M <= 0 || N <= 0)
        return SELD_ERR_INVALID;
    TnJobs jobs = {};
    for (int j = 0; j < njobs; ++j) {
        if (!A[j] || !Bm[j] || !C[j] || (want_bias && !colsum[j])) return SELD_ERR_INVALID;
        jobs.A[j] = A[j]; jobs.B[j] = Bm[j]; jobs.lda[j] = lda[j]; jobs.shift[j] = shift[j]; jobs.out_w[j] = C[j]; jobs.out_b[j] = want_bias ? colsum[j] : nullptr;
    }
    Scratch s;
    const int64_t per = (int64_t)128 * N + N;
    // the launcher takes at most one split per 160 rows (rounding the rows of a split up to whole chunks only lowers the count)
    float* slab = s.get((size_t)njobs * std::min(gemm_tn_max_splits(), (M + 159) / 160) * per);
    if (!slab) return SELD_ERR_NOMEM;
    int ns = 0;
    if (launch_gemm_tn_sb_batch(0, k_kc, jobs, njobs, ldb, slab, &ns, M, N, S, want_bias)) return SELD_ERR_INVALID;
    launch_reduce_slabs2_batch(0, slab, ns, per, jobs, njobs, (int64_t)128 * N, want_bias ? N : 0);
    *nslab = ns;
    return done();
}

// tile mode (K1 % 128 == 0, optionally the implicit im2col of a 3x3 kernel gradient): slab_cap floats of slab space limit the splits
int seld_k_gemm_tn_sb_tiles(const float* A, int lda, const float* Bm, int ldb, float* C, int M, int K1, int N, int64_t slab_cap, int conv_C, int conv_H,
                            int conv_W, int* nslab) {
    if (!A || !Bm || !C || !nslab || slab_cap < 1 || slab_cap > ((int64_t)1 << 28)) return SELD_ERR_INVALID;
    Scratch s;
    float* slab = s.get((size_t)slab_cap);
    if (!slab) return SELD_ERR_NOMEM;
    int ns = 0;
    if (launch_gemm_tn_sb_tiles(0, k_kc, A, lda, Bm, ldb, slab, slab_cap, &ns, M, K1, N, conv_C, conv_H, conv_W)) return SELD_ERR_INVALID;
    launch_reduce_slabs2(0, slab, ns, (int64_t)K1 * N, C, (int64_t)K1 * N, nullptr, 0);
    *nslab = ns;
    return done();
}

int seld_k_reduce_slabs_groups(int nslab) { return reduce_slabs_groups(nslab); }

// which 0: out_w[n_w] (+)= sum of slabs; 1: [out_w n_w | out_b n_b] = sum of slabs; 2: two stages through tmp [seld_k_reduce_slabs_groups(nslab)][n_w]
int seld_k_reduce_slabs_ex(int which, const float* slab, int nslab, int64_t stride, float* out_w, int64_t n_w, float* out_b, int64_t n_b, int accumulate,
                           float* tmp) {
    if (!slab || !out_w || nslab < 1 || n_w < 1 || n_b < 0 || stride < n_w + n_b || which < 0 || which > 2) return SELD_ERR_INVALID;
    if ((which == 1) != (n_b > 0) || (n_b > 0 && !out_b) || (which != 0 && accumulate) || (which == 2 && !tmp)) return SELD_ERR_INVALID;
    if (which == 0) launch_reduce_slabs(0, slab, nslab, stride, out_w, n_w, accumulate);
    else if (which == 1) launch_reduce_slabs2(0, slab, nslab, stride, out_w, n_w, out_b, n_b);
    else launch_reduce_slabs_2stage(0, slab, nslab, stride, out_w, n_w, tmp);
    return done();
}

// job j's slabs follow job j - 1's (nslab slabs each), as launch_gemm_tn_sb_batch leaves them
int seld_k_reduce_slabs2_batch(const float* slab, int nslab, int64_t stride, int njobs, float* const* out_w, float* const* out_b, int64_t n_w, int64_t n_b) {
    if (!slab || !out_w || nslab < 1 || njobs < 1 || njobs > TN_MAX_JOBS || n_w < 1 || n_b < 0 || stride < n_w + n_b || (n_b > 0 && !out_b)) return SELD_ERR_INVALID;
    TnJobs jobs = {};
    for (int j = 0; j < njobs; ++j) {
        if (!out_w[j] || (n_b > 0 && !out_b[j])) return SELD_ERR_INVALID;
        jobs.out_w[j] = out_w[j]; jobs.out_b[j] = n_b > 0 ? out_b[j] : nullptr;
    }
    launch_reduce_slabs2_batch(0, slab, nslab, stride, jobs, njobs, n_w, n_b);
    return done();
}

// w1, b1, w2, b2, n: arrays of two (the SED head, the DOA head); weff [K + 1][n[0] + n[1]]
int seld_k_heads_weff(const float* const* w1, const float* const* b1, const float* const* w2, const float* const* b2, const int* n, int K, int Hd, float* weff) {
    if (!w1 || !b1 || !w2 || !b2 || !n || !weff || K < 1 || Hd < 1 || n[0] < 1 || n[1] < 1) return SELD_ERR_INVALID;
    if (launch_heads_weff(0, w1, b1, w2, b2, n, K, Hd, weff)) return SELD_ERR_INVALID;
    return done();
}

int seld_k_heads_grad(const float* const* w1, const float* const* b1, const float* const* w2, float* const* dw1, float* const* db1, float* const* dw2,
                      float* const* db2, const int* n, int K, int Hd, const float* F, const float* cs) {
    if (!w1 || !b1 || !w2 || !dw1 || !db1 || !dw2 || !db2 || !n || !F || !cs || K < 1 || Hd < 1 || n[0] < 1 || n[1] < 1 || n[0] + n[1] > 64) return SELD_ERR_INVALID;
    if (launch_heads_grad(0, w1, b1, w2, dw1, db1, dw2, db2, n, K, Hd, F, cs)) return SELD_ERR_INVALID;
    return done();
}

// the merged pre-pass launch (prep.hip) into the *_fused targets and the three stand-alone launches into the *_alone ones, from the same inputs:
// na GEMM weight splits (dst: 3 K N bf16 each), nb 64 -> 64 conv weight splits (dst: 9 * 3 * 4096 bf16 each), the folded head weights (weff_fused
// NULL: off).  Nothing to do (0, 0, off) launches nothing.
int seld_k_weight_prep(int na, const float* const* a_src, const int* a_ldb, const int* a_transb, const int* a_K, const int* a_N,
                       unsigned short* const* a_fused, unsigned short* const* a_alone, int nb, const float* const* b_w, const int* b_flip,
                       unsigned short* const* b_fused, unsigned short* const* b_alone, const float* const* w1, const float* const* b1,
                       const float* const* w2, const float* const* b2, const int* n, int K, int Hd, float* weff_fused, float* weff_alone) {
    if (na < 0 || nb < 0 || (na && (!a_src || !a_ldb || !a_transb || !a_K || !a_N || !a_fused || !a_alone)) || (nb && (!b_w || !b_flip || !b_fused || !b_alone)))
        return SELD_ERR_INVALID;
    if (weff_fused && (!weff_alone || !w1 || !b1 || !w2 || !b2 || !n)) return SELD_ERR_INVALID;
    GemmSplitJobs a = {};
    SplitWeightJobs b = {};
    HeadsLin h = {};
    a.njobs = na;
    for (int i = 0; i < na && i < GSB_MAX_JOBS; ++i) {
        a.src[i] = a_src[i]; a.dst[i] = a_fused[i]; a.ldb[i] = a_ldb[i]; a.transb[i] = a_transb[i]; a.K[i] = a_K[i]; a.N[i] = a_N[i];
    }
    for (int i = 0; i < nb && i < 8; ++i) { b.w[i] = b_w[i]; b.dst[i] = b_fused[i]; b.flip[i] = b_flip[i]; }
    if (weff_fused) {
        for (int i = 0; i < 2; ++i) { h.w1[i] = w1[i]; h.b1[i] = b1[i]; h.w2[i] = w2[i]; h.b2[i] = b2[i]; h.n[i] = n[i]; }
        h.K = K; h.Hd = Hd;
    }
    if (launch_weight_prep(0, k_kc, a, na, b, nb, h, weff_fused)) return SELD_ERR_INVALID;
    if (na && launch_gemm_split_b(0, k_kc, na, a_src, a_alone, a_ldb, a_transb, a_K, a_N)) return SELD_ERR_INVALID;
    if (nb && launch_split_weights_batch(0, k_kc, nb, b_w, b_alone, b_flip)) return SELD_ERR_INVALID;
    if (weff_fused && launch_heads_weff(0, w1, b1, w2, b2, n, K, Hd, weff_alone)) return SELD_ERR_INVALID;
    return done();
}

int seld_k_mul(const float* a, const float* b, float* out, int64_t n) {
    if (!a || !b || !out || n < 1 || !al16(a) || !al16(b) || !al16(out)) return SELD_ERR_INVALID;
    if (launch_mul(0, a, b, out, n)) return SELD_ERR_INVALID;
    return done();
}

int seld_device_clocks(int device, int* compute_units, int* clock_khz, int* mem_clock_khz, int* mem_bus_bits) {
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, device) != hipSuccess) return SELD_ERR_HIP;
    if (compute_units) *compute_units = p.multiProcessorCount;
    if (clock_khz) *clock_khz = p.clockRate;
    if (mem_clock_khz) *mem_clock_khz = p.memoryClockRate;
    if (mem_bus_bits) *mem_bus_bits = p.memoryBusWidth;
    return SELD_OK;
}

}  // extern "C"
