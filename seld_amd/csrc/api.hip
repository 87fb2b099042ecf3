// api.hip — C ABI of libseld_hip.so (include/seld_hip.h): context creation, options, variable layout, host copies, the losses and the
// step entry points.  The passes they call are in forward.hip / backward.hip, data parallelism in dp.hip; ctx.h is what they share.
#include "ctx.h"

#include <algorithm>
#include <math.h>
#include <stdio.h>
#include <string.h>

static std::string g_create_err;

int fail(seld_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg; else g_create_err = msg;
    return code;
}

static void add_var(std::vector<Var>& v, int64_t& off, const std::string& name, std::initializer_list<int64_t> shape) {
    Var x;
    x.name = name;
    x.off = off;
    x.rank = (int)shape.size();
    int64_t n = 1;
    int i = 0;
    for (int k = 0; k < 4; ++k) x.shape[k] = 1;
    for (auto s : shape) { x.shape[i++] = s; n *= s; }
    off += n;
    v.push_back(x);
}

int check_launch(seld_ctx* c, const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(c, SELD_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
    return 0;
}

// side stream: everything enqueued on it after this call starts once the main stream has reached this point
void fork_side(seld_ctx* c) {
    hipEventRecord(c->ev_fork, c->stream);
    hipStreamWaitEvent(c->side, c->ev_fork, 0);
}
// Which products run on the split-bf16 GEMM: shapes gemm_sb.hip handles (K % 32 == 0, N % 128 == 0); anything else stays
// on the exact-fp32 MFMA GEMM.  The same predicates gate the forward product and its input gradient.
bool gru_sb(const seld_ctx* c, const GruL& G) { return c->gemm_split_bf16 && (G.in_feat % 128) == 0; }
// simple_dense_block with kernel_size > 1 or dropout_rate > 0 on a hidden layer: the heads run layer by layer (no shared first product,
// no W1 W2 fold)
bool heads_general(const seld_ctx* c) {
    for (int hd = 0; hd < 2; ++hd)
        for (const DenseL& D : c->heads[hd].layers) if (D.ks > 1 || D.rate > 0.f) return true;
    return false;
}

bool heads_sb(const seld_ctx* c) {
    const DenseL &S0 = c->heads[0].layers[0], &D0 = c->heads[1].layers[0];
    return !heads_general(c) && c->gemm_split_bf16 && c->heads[0].layers.size() > 1 && c->heads[1].layers.size() > 1 && S0.in == D0.in && S0.out == D0.out &&
           (S0.in % 128) == 0 && (S0.out % 128) == 0;
}

// Heads of the form Dense(h, linear) -> Dense(n, act) on shared features (seldnet.json: Conv1D(128, 1) then the output Dense):
// y = act(feat (W1 W2) + (b1 W2 + b2)).  The 128-wide hidden tensor is never formed, forward or backward: the products
// shrink from K = N = 128 to N = 12 + 36 columns in one launch, and all four weight gradients of a head follow from
// F = feat^T dy and colsum(dy) (gemm.hip, heads_grad_kernel).  Same mathematics, different association of the fp32 sums.
bool heads_lin(const seld_ctx* c) {
    const Head &Hs = c->heads[0], &Hdo = c->heads[1];
    if (!c->heads_fused || Hs.layers.size() != 2 || Hdo.layers.size() != 2 || Hs.hidden_act || Hdo.hidden_act || heads_general(c)) return false;   // W1 W2 folds only without an activation between them
    const DenseL &S0 = Hs.layers[0], &D0 = Hdo.layers[0];
    return S0.in == D0.in && S0.out == D0.out && Hs.layers[1].out + Hdo.layers[1].out <= 64 && (S0.in & 3) == 0 &&
           ((Hs.layers[1].out + Hdo.layers[1].out) & 3) == 0;
}

// the 3x3 convolution of a stage-1 bottleneck (64 -> 64 channels on a width conv_sb.hip / conv_wgrad_sb.hip have kernels for)
// ... of a stage-2 / 3 bottleneck: split-bf16 products on im2col rows formed on load (no col tensor)
bool rn_c1_implicit(const seld_ctx* c, const RnBlock& R) { return c->rn_implicit3x3 && R.c[1].wsp && R.c[1].wsp_t && rn_conv3_sb_ok(R.w, R.w); }
// (stage 0: 32 -> 32 channels as 64 -> 64 over pairs of bins, rn_c1_width = the width the kernels see)
int rn_c1_width(const RnBlock& R) { return R.c[1].w2 ? R.Wout / 2 : R.Wout; }
bool rn_c1_direct(const RnBlock& R) {
    const int W = rn_c1_width(R);
    return R.c[1].wsp9 && (!R.c[1].w2 || (R.Wout & 1) == 0) && (W == 16 || W == 8 || W == 4);
}

extern "C" {

int seld_abi_sizes(int32_t* out, int n) {
    const int32_t v[2] = {(int32_t)sizeof(seld_arch), (int32_t)sizeof(seld_loss_cfg)};
    for (int i = 0; out && i < n && i < 2; ++i) out[i] = v[i];
    return 2;
}

const char* seld_last_error(const seld_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

int seld_create(const seld_arch* a, int B, int T, int dtype, int device, seld_ctx** out) {
    if (!a || !out) return fail(nullptr, SELD_ERR_INVALID, "null argument");
    *out = nullptr;
    if (dtype != SELD_DTYPE_F32 && dtype != SELD_DTYPE_BF16) return fail(nullptr, SELD_ERR_UNSUPPORTED, "dtype must be SELD_DTYPE_F32 or SELD_DTYPE_BF16");
    if (B <= 0 || T <= 0) return fail(nullptr, SELD_ERR_INVALID, "B and T must be positive");
    if (a->n_conv < 1 || a->n_conv > SELD_MAX_LAYERS || a->n_gru < 1 || a->n_gru > SELD_MAX_LAYERS ||
        a->n_sed_dense < 0 || a->n_sed_dense > SELD_MAX_LAYERS || a->n_doa_dense < 0 || a->n_doa_dense > SELD_MAX_LAYERS)
        return fail(nullptr, SELD_ERR_INVALID, "layer counts out of range");
    if (a->in_ch != 7 && a->in_ch != 10)
        return fail(nullptr, SELD_ERR_UNSUPPORTED, "first conv kernels are built for in_ch = 7 (foa) and 10 (mic)");
    if (a->n_freq != 64) return fail(nullptr, SELD_ERR_UNSUPPORTED, "first conv kernel is built for n_freq = 64");
    if (a->n_classes <= 0) return fail(nullptr, SELD_ERR_INVALID, "n_classes must be positive");
    const bool xcep = a->first_kind == SELD_FIRST_XCEPTION, resn = a->first_kind == SELD_FIRST_RESNET50;
    if (a->first_kind != SELD_FIRST_SIMPLE_CONV && !xcep && !resn) return fail(nullptr, SELD_ERR_UNSUPPORTED, "unknown FIRST block kind");
    if (!(a->conv_dropout >= 0.f && a->conv_dropout < 1.f) || !(a->gru_dropout >= 0.f && a->gru_dropout < 1.f))
        return fail(nullptr, SELD_ERR_INVALID, "conv_dropout / gru_dropout: 0 <= rate < 1");
    if (a->conv_dropout > 0.f && a->first_kind != SELD_FIRST_SIMPLE_CONV)
        return fail(nullptr, SELD_ERR_UNSUPPORTED, "conv_dropout: simple_conv_block only (the other FIRST blocks' specs have no Dropout)");
    if (resn) {
        if (a->n_conv != 1 || a->pool_t[0] != 5 || a->pool_f[0] != 4 || a->rn_filters != 32)
            return fail(nullptr, SELD_ERR_UNSUPPORTED, "resnet50_block: one entry conv2d_bn(64) with pool (5,4), filters 32 (spec/RESNET50_BLOCK.md)");
        for (int s_ = 0; s_ < 4; ++s_)
            if (a->rn_blocks[s_] < 1 || a->rn_blocks[s_] > 8) return fail(nullptr, SELD_ERR_UNSUPPORTED, "resnet50_block: 1..8 blocks per stage");
    }
    if (xcep && (a->n_conv != 1 || a->pool_t[0] != 5 || a->pool_f[0] != 4 || a->xc_blocks < 1 || a->xc_blocks > SELD_MAX_XC_BLOCKS))
        return fail(nullptr, SELD_ERR_UNSUPPORTED, "xception_block: one entry conv2d_bn(64) with pool (5,4) and 1..16 middle modules (spec/XCEPTION_BLOCK.md)");
    int H = T, W = a->n_freq;
    for (int i = 0; i < a->n_conv; ++i) {
        if (a->filters[i] != 64) return fail(nullptr, SELD_ERR_UNSUPPORTED, "conv kernels are built for 64 filters");
        if (a->pool_t[i] <= 0 || a->pool_f[i] <= 0 || H % a->pool_t[i] || W % a->pool_f[i])
            return fail(nullptr, SELD_ERR_UNSUPPORTED, "time/frequency extents must be divisible by the pool sizes");
        if (i > 0 && !(W == 2 || W == 4 || W == 8 || W == 16 || W == 32))
            return fail(nullptr, SELD_ERR_UNSUPPORTED, "inner conv width must be a power of two <= 32");
        H /= a->pool_t[i];
        W /= a->pool_f[i];
    }
    if (xcep) {
        if (W != 16) return fail(nullptr, SELD_ERR_UNSUPPORTED, "xception_block: 16 frequency bins after the entry pool (n_freq 64)");
        W /= 8;       // exit MaxPooling2D((1, 8))
    }
    if (resn && W != 16) return fail(nullptr, SELD_ERR_UNSUPPORTED, "resnet50_block: 16 frequency bins after the entry pool (n_freq 64)");
    const int S = H, feat = resn ? (W / 8) * 32 * a->rn_filters : W * 64;
    for (int i = 0; i < a->n_gru; ++i)
        if (a->gru_units[i] != 128) return fail(nullptr, SELD_ERR_UNSUPPORTED, "GRU kernels are built for 128 units");
    if (feat <= 0 || feat % 128) return fail(nullptr, SELD_ERR_UNSUPPORTED, "GRU input projection expects a multiple of 128 features (seldnet.json: F'*C' = 2*64)");

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(nullptr, SELD_ERR_HIP, "no HIP device");
    if (device < 0 || device >= ndev) return fail(nullptr, SELD_ERR_INVALID, "bad device index");
    if (hipSetDevice(device) != hipSuccess) return fail(nullptr, SELD_ERR_HIP, "hipSetDevice failed");

    seld_ctx* c = new seld_ctx();
    c->arch = *a; c->B = B; c->Bmax = B; c->T = T; c->S = S; c->device = device;
    c->kc.mfma_one = dtype == SELD_DTYPE_BF16;

    // ---- variable layout (Keras creation order; oracle/seldnet_oracle.py::variable_specs is the twin)
    int64_t off = 0, soff = 0;
    int cin = a->in_ch;
    H = T; W = a->n_freq;
    for (int i = 0; i < a->n_conv; ++i) {
        ConvL L;
        L.H = H; L.W = W; L.Cin = cin; L.pt = a->pool_t[i]; L.pf = a->pool_f[i];
        char nm[64];
        snprintf(nm, sizeof nm, "conv%d.kernel", i); L.w_off = off; add_var(c->tr, off, nm, {3, 3, cin, 64});
        snprintf(nm, sizeof nm, "conv%d.bias", i);   L.b_off = off; add_var(c->tr, off, nm, {64});
        snprintf(nm, sizeof nm, "bn%d.gamma", i);    L.g_off = off; add_var(c->tr, off, nm, {64});
        snprintf(nm, sizeof nm, "bn%d.beta", i);     L.be_off = off; add_var(c->tr, off, nm, {64});
        snprintf(nm, sizeof nm, "bn%d.moving_mean", i);     L.mm_off = soff; add_var(c->nt, soff, nm, {64});
        snprintf(nm, sizeof nm, "bn%d.moving_variance", i); L.mv_off = soff; add_var(c->nt, soff, nm, {64});
        c->conv.push_back(L);
        cin = 64; H /= L.pt; W /= L.pf;
    }
    if (xcep)
        for (int b = 0; b < a->xc_blocks; ++b)
            for (int u = 0; u < 3; ++u) {
                XcUnit U;
                char nm[64];
                snprintf(nm, sizeof nm, "xc%d.%d.depthwise_kernel", b, u); U.dw_off = off; add_var(c->tr, off, nm, {3, 3, 64, 1});
                snprintf(nm, sizeof nm, "xc%d.%d.pointwise_kernel", b, u); U.pw_off = off; add_var(c->tr, off, nm, {1, 1, 64, 64});
                snprintf(nm, sizeof nm, "xc%d.%d.gamma", b, u); U.g_off = off; add_var(c->tr, off, nm, {64});
                snprintf(nm, sizeof nm, "xc%d.%d.beta", b, u); U.be_off = off; add_var(c->tr, off, nm, {64});
                snprintf(nm, sizeof nm, "xc%d.%d.moving_mean", b, u); U.mm_off = soff; add_var(c->nt, soff, nm, {64});
                snprintf(nm, sizeof nm, "xc%d.%d.moving_variance", b, u); U.mv_off = soff; add_var(c->nt, soff, nm, {64});
                c->xc.push_back(U);
            }
    if (resn) {
        int cin_b = 64, wcur = 16;
        for (int s_ = 0; s_ < 4; ++s_) {
            const int wd = a->rn_filters << s_;
            for (int b = 0; b < a->rn_blocks[s_]; ++b) {
                RnBlock R;
                R.Cin = cin_b; R.w = wd; R.stride_f = (b == 0 && s_ > 0) ? 2 : 1; R.Win = wcur; R.Wout = wcur / R.stride_f; R.proj = b == 0;
                auto mk = [&](RnConv& cv, const char* tag, int k, int ci, int co) {
                    char nm[96];
                    cv.k = k; cv.Cin = ci; cv.Cout = co;
                    snprintf(nm, sizeof nm, "rn%d.%d.%s.kernel", s_, b, tag); cv.w_off = off; add_var(c->tr, off, nm, {k, k, ci, co});
                    snprintf(nm, sizeof nm, "rn%d.%d.%s.gamma", s_, b, tag); cv.g_off = off; add_var(c->tr, off, nm, {co});
                    snprintf(nm, sizeof nm, "rn%d.%d.%s.beta", s_, b, tag); cv.be_off = off; add_var(c->tr, off, nm, {co});
                    snprintf(nm, sizeof nm, "rn%d.%d.%s.moving_mean", s_, b, tag); cv.mm_off = soff; add_var(c->nt, soff, nm, {co});
                    snprintf(nm, sizeof nm, "rn%d.%d.%s.moving_variance", s_, b, tag); cv.mv_off = soff; add_var(c->nt, soff, nm, {co});
                };
                mk(R.c[0], "c0", 1, cin_b, wd); mk(R.c[1], "c1", 3, wd, wd); mk(R.c[2], "c2", 1, wd, 4 * wd);
                if (R.proj) mk(R.sc, "sc", 1, cin_b, 4 * wd);
                c->rn.push_back(R);
                cin_b = 4 * wd; wcur = R.Wout;
            }
        }
        c->rn_feat = feat;
    }
    int fin = feat;
    for (int i = 0; i < a->n_gru; ++i) {
        GruL G;
        G.in_feat = fin;
        const char* dn[2] = {"fwd", "bwd"};
        for (int d = 0; d < 2; ++d) {
            char nm[64];
            snprintf(nm, sizeof nm, "gru%d.%s.kernel", i, dn[d]);           G.k_off[d] = off; add_var(c->tr, off, nm, {fin, 384});
            snprintf(nm, sizeof nm, "gru%d.%s.recurrent_kernel", i, dn[d]); G.u_off[d] = off; add_var(c->tr, off, nm, {128, 384});
            snprintf(nm, sizeof nm, "gru%d.%s.bias", i, dn[d]);             G.b_off[d] = off; add_var(c->tr, off, nm, {2, 384});
        }
        c->gru.push_back(G);
        fin = 128;
    }
    for (int hd = 0; hd < 2; ++hd) {
        const char* hn = hd == 0 ? "sed" : "doa";
        const int nd = hd == 0 ? a->n_sed_dense : a->n_doa_dense;
        const int32_t* units = hd == 0 ? a->sed_units : a->doa_units;
        int in = fin;
        for (int j = 0; j < nd; ++j) {
            if (units[j] <= 0 || (units[j] & 3)) { delete c; return fail(nullptr, SELD_ERR_UNSUPPORTED, "dense units must be a positive multiple of 4"); }
            DenseL D; D.out = units[j];
            D.ks = std::max(1, hd == 0 ? a->sed_kernel_size : a->doa_kernel_size);
            D.rate = hd == 0 ? a->sed_dropout : a->doa_dropout;
            if (D.ks > 15 || !(D.rate >= 0.f && D.rate < 1.f)) { delete c; return fail(nullptr, SELD_ERR_UNSUPPORTED, "simple_dense_block: kernel_size 1..15, 0 <= dropout_rate < 1"); }
            D.in_base = in; D.in = D.ks * in; D.drop_id = (unsigned)(16 * hd + j);
            char nm[64];
            snprintf(nm, sizeof nm, "%s.dense%d.kernel", hn, j); D.w_off = off; add_var(c->tr, off, nm, {D.ks, in, units[j]});
            snprintf(nm, sizeof nm, "%s.dense%d.bias", hn, j);   D.b_off = off; add_var(c->tr, off, nm, {units[j]});
            c->heads[hd].layers.push_back(D);
            in = units[j];
        }
        DenseL D; D.in = D.in_base = in; D.out = (hd == 0 ? 1 : 3) * a->n_classes;
        char nm[64];
        snprintf(nm, sizeof nm, "%s.out.kernel", hn); D.w_off = off; add_var(c->tr, off, nm, {in, D.out});
        snprintf(nm, sizeof nm, "%s.out.bias", hn);   D.b_off = off; add_var(c->tr, off, nm, {D.out});
        c->heads[hd].layers.push_back(D);
        c->heads[hd].act = hd == 0 ? 1 : 2;
        c->heads[hd].hidden_act = hd == 0 ? a->sed_dense_act : a->doa_dense_act;
        if (c->heads[hd].hidden_act < SELD_ACT_NONE || c->heads[hd].hidden_act > SELD_ACT_RELU) { delete c; return fail(nullptr, SELD_ERR_UNSUPPORTED, "dense_activation: none, sigmoid, tanh or relu"); }
    }
    c->nparam = off; c->nstate = soff;

    // ---- device memory
#define ALLOC(ptr, n) do { int rc_ = dalloc(c, &(ptr), (size_t)(n)); if (rc_) { g_create_err = c->err; seld_destroy(c); return rc_; } } while (0)
    ALLOC(c->params, c->nparam); ALLOC(c->grads, c->nparam); ALLOC(c->adam_m, c->nparam); ALLOC(c->adam_v, c->nparam);
    ALLOC(c->state, c->nstate);
    hipMemset(c->params, 0, c->nparam * 4); hipMemset(c->grads, 0, c->nparam * 4);
    hipMemset(c->adam_m, 0, c->nparam * 4); hipMemset(c->adam_v, 0, c->nparam * 4); hipMemset(c->state, 0, c->nstate * 4);
    ALLOC(c->small, (size_t)a->n_conv * 64 * 6);
    size_t zmax = 0;
    for (int i = 0; i < a->n_conv; ++i) {
        ConvL& L = c->conv[i];
        const size_t nz = (size_t)B * L.H * L.W * 64;
        const size_t np = (size_t)B * (L.H / L.pt) * (L.W / L.pf) * 64;
        ALLOC(L.z, nz); ALLOC(L.p, np); ALLOC(L.dp, np);
        if (a->conv_dropout > 0.f) ALLOC(L.pd, np);
        if (i == 0) { float* am = nullptr; ALLOC(am, (np + 3) / 4); L.amax = reinterpret_cast<unsigned char*>(am); ALLOC(L.zext, np); }
        if (i == 1 && L.W == 16 && L.pt == 1 && L.pf == 4) ALLOC(L.zext, np);      // the (1,4) windows' extremes of z (conv_sb.hip EXT), when the third block's loader pools
        if (nz > zmax) zmax = nz;
        float* sm = c->small + (size_t)i * 64 * 6;
        L.mean = sm; L.invstd = sm + 64; L.scale = sm + 128; L.shift = sm + 192; L.c1c2 = sm + 256;
    }
    ALLOC(c->dzbuf, zmax);
    {
        const size_t kp = (size_t)conv_gram_dim(c->conv[0].Cin);
        ALLOC(c->gram_slab, (size_t)conv_gram_slab_capacity() * kp * kp);
        ALLOC(c->gram, kp * kp);
        ALLOC(c->mmat, kp * 64);
    }
    if (xcep) {
        const size_t npx = (size_t)B * S * 16 * 64;     // elements of one [B,S,16,64] tensor
        ALLOC(c->xc_small, c->xc.size() * 64 * 6);
        ALLOC(c->xc_ident, 64 * 6);
        launch_xc_ident(0, c->xc_ident);
        for (size_t i = 0; i < c->xc.size(); ++i) {
            XcUnit& U = c->xc[i];
            ALLOC(U.dwo, npx); ALLOC(U.z, npx);
            if (i % 3 != 2) ALLOC(U.a, npx);
            float* sm = c->xc_small + i * 64 * 6;
            U.mean = sm; U.invstd = sm + 64; U.scale = sm + 128; U.shift = sm + 192; U.c1c2 = sm + 256;
        }
        c->xc_x.resize(a->xc_blocks + 1);
        c->xc_x[0] = c->conv[0].p;
        for (int b = 1; b <= a->xc_blocks; ++b) ALLOC(c->xc_x[b], npx);
        for (int k = 0; k < 4; ++k) ALLOC(c->xc_g[k], npx);
        ALLOC(c->xc_dz2, npx);
        ALLOC(c->xc_feat, (size_t)B * S * 128);
        ALLOC(c->xc_part, (size_t)xc_partial_capacity() * 128);
        {   // depthwise kernel-gradient slabs: dw3x3_bwd_w's (<= xc_partial_capacity()) or, with xc_fused_dw_bwd, one per 4 image rows, two buffers
            // (a unit's combine on the side stream reads one while the next unit's input-gradient kernel fills the other)
            const size_t per = (size_t)std::max(xc_partial_capacity(), xc_dw_fused_slabs(c->Bmax, c->S)) * 576;
            ALLOC(c->xc_slab, 2 * per);
            c->xc_slab_per = per;
            ALLOC(c->xc_part_dw, (size_t)xc_dw_fused_slabs(c->Bmax, c->S) * 128);
            ALLOC(c->xc_slab_tmp, (size_t)reduce_slabs_groups(xc_dw_fused_slabs(c->Bmax, c->S)) * 576);
            // xc_nowait (round 5): every unit its OWN slab buffers — [pointwise slabs | depthwise slabs | first-stage sums], ~20 MB per unit — so that no buffer
            // is written twice in a step and the backward loop needs no hand-over events (each wait costs the main stream ~5-10 us of bubble, 2 per unit)
            c->xc_unit_slab_pw = (size_t)xc_pw_bwd_slabs() * 4096;
            c->xc_unit_slab_dw = (size_t)xc_dw_fused_slabs(c->Bmax, c->S) * 576;
            c->xc_unit_slab_per = c->xc_unit_slab_pw + c->xc_unit_slab_dw + (size_t)reduce_slabs_groups(xc_dw_fused_slabs(c->Bmax, c->S)) * 576 +
                                  (size_t)reduce_slabs_groups(xc_pw_bwd_slabs()) * 4096;      // + the two combines' first-stage sums
            ALLOC(c->xc_unit_slab, c->xc.size() * c->xc_unit_slab_per);
        }
    }
    if (resn) {
        size_t mx_out = 0, mx_w = 0, mx_col = 0, mx_in = (size_t)B * S * 16 * 64;
        for (auto& R : c->rn) {
            const size_t M = (size_t)B * S * R.Wout;
            for (int i = 0; i < 3; ++i) { ALLOC(R.c[i].z, M * R.c[i].Cout); ALLOC(R.c[i].coef, (size_t)6 * R.c[i].Cout); }
            if (R.proj) { ALLOC(R.sc.z, M * 4 * R.w); ALLOC(R.sc.coef, (size_t)6 * 4 * R.w); }
            ALLOC(R.y0, M * R.w); ALLOC(R.y1, M * R.w); ALLOC(R.out, M * 4 * R.w); ALLOC(R.gate, M * R.w);
            mx_out = std::max(mx_out, M * 4 * R.w); mx_w = std::max(mx_w, M * R.w); mx_col = std::max(mx_col, M * 9 * R.w);
            mx_in = std::max(mx_in, (size_t)B * S * R.Win * R.Cin);
        }
        for (auto& R : c->rn)
            for (RnConv* cv : {&R.c[0], &R.c[1], &R.c[2], &R.sc}) {
                const int K = cv->k * cv->k * cv->Cin, N = cv->Cout;
                if (!N) continue;
                if (rn_sb_fwd_ok(K, N)) ALLOC(cv->wsp, gemm_sb_split_elems(K, N));
                if (rn_sb_dgrad_ok(K, N)) ALLOC(cv->wsp_t, gemm_sb_split_elems(K, N));
                if (cv->k == 3 && ((cv->Cin == 64 && N == 64) || (cv->Cin == 32 && N == 32))) {
                    ALLOC(cv->wsp9, (size_t)9 * 3 * 4096); ALLOC(cv->wsp9_flip, (size_t)9 * 3 * 4096);
                    if (N == 32) { ALLOC(cv->w2, (size_t)9 * 4096); ALLOC(cv->dw2, (size_t)9 * 4096); }
                }
            }
        // BatchNorm partials: the most floats any launch writes into rn_part / rn_part_side at Bmax — a product's epilogue statistics
        // (rn_epi_partial_floats), the separate statistics pass and its backward (rn_stats_partial_floats), stage 1's direct 3x3 conv (one 64-channel
        // chunk, at most conv_sb_partial_capacity() workgroups)
        size_t npart = (size_t)conv_sb_partial_capacity() * 128;
        for (auto& R : c->rn)
            for (RnConv* cv : {&R.c[0], &R.c[1], &R.c[2], &R.sc})
                if (cv->Cout) npart = std::max({npart, rn_epi_partial_floats((int64_t)B * S * R.Wout, cv->Cout), rn_stats_partial_floats(cv->Cout)});
        c->rn_part_floats = npart;
        ALLOC(c->rn_part, npart);
        ALLOC(c->rn_part_side, npart);
        ALLOC(c->rn_gx[0], mx_in); ALLOC(c->rn_gx[1], mx_in);
        for (auto& b_ : c->rn_bz) ALLOC(b_, mx_out);
        for (auto& b_ : c->rn_bb) ALLOC(b_, mx_w);
        ALLOC(c->rn_ba, mx_w);
        c->rn_col_elems = mx_col;      // the im2col tensors (a block's col, the shared dcol) are allocated on first use: no default path needs them
        ALLOC(c->rn_w9_slab, (size_t)conv_wgrad_slab_capacity() * (9 * 4096 + 64));
    }
    if (resn || a->first_kind == SELD_FIRST_XCEPTION) {
        bool ok_ = hipEventCreateWithFlags(&c->ev_rn_ready, hipEventDisableTiming | hipEventDisableSystemFence) == hipSuccess;
        for (auto& e_ : c->ev_rn_free) ok_ = ok_ && hipEventCreateWithFlags(&e_, hipEventDisableTiming | hipEventDisableSystemFence) == hipSuccess;
        if (!ok_) { seld_destroy(c); return fail(nullptr, SELD_ERR_HIP, "event creation failed"); }
    }
    ALLOC(c->stat_partial, (size_t)conv_stat_partial_capacity() * 128);
    ALLOC(c->bn_partial, (size_t)bn_partial_capacity() * 128);
    ALLOC(c->wgrad_slab, (size_t)conv_wgrad_slab_capacity() * (9 * 4096 + 64));
    if (a->n_conv >= 2 && c->xc.empty() && c->rn.empty()) {      // option conv_wgrad_side (simple_conv_block: the second / third block's kernel gradients beside the main chain)
        ALLOC(c->wgrad_slab_side, (size_t)conv_wgrad_slab_capacity() * (9 * 4096 + 64));
        ALLOC(c->dzbuf_alt, zmax);
        for (int k_ = 0; k_ < 2; ++k_)      // ev_rn_free[0 / 1]: the side-stream reader of dzbuf / dzbuf_alt is done (the block models create all five for their own slots)
            if (!c->ev_rn_free[k_] && hipEventCreateWithFlags(&c->ev_rn_free[k_], hipEventDisableTiming | hipEventDisableSystemFence) != hipSuccess) {
                seld_destroy(c); return fail(nullptr, SELD_ERR_HIP, "event creation failed");
            }
    }
    ALLOC(c->tn_slab, (size_t)tn_slab_capacity());
    ALLOC(c->cs_slab, (size_t)256 * 512);
    ALLOC(c->wflip, 9 * 4096);
    ALLOC(c->wsplit, (size_t)2 * c->conv.size() * 9 * 3 * 4096);
    for (size_t i = 0; i < c->conv.size(); ++i) {
        c->wsp_fwd[i] = c->wsplit + (2 * i) * 9 * 3 * 4096;
        c->wsp_bwd[i] = c->wsplit + (2 * i + 1) * 9 * 3 * 4096;
    }
    const size_t rows = (size_t)B * S;
    for (int i = 0; i < a->n_gru; ++i) {
        GruL& G = c->gru[i];
        for (int d = 0; d < 2; ++d) { ALLOC(G.gx[d], rows * 384); ALLOC(G.sv[d], rows * 512); ALLOC(G.h[d], rows * 128); }
        ALLOC(G.out, rows * 128); ALLOC(G.din, rows * (size_t)G.in_feat);
        if (a->gru_dropout > 0.f) {
            for (int d = 0; d < 2; ++d) {
                ALLOC(G.imask[d], (size_t)B * G.in_feat); ALLOC(G.rmask[d], (size_t)B * 128);
                ALLOC(G.xm[d], rows * (size_t)G.in_feat); ALLOC(G.hm[d], rows * 128);
            }
            ALLOC(G.dtmp, rows * (size_t)G.in_feat);
            if (!c->ones) { ALLOC(c->ones, (size_t)B * 2048); launch_fill(0, c->ones, (int64_t)B * 2048, 1.f); }
        }
    }
    ALLOC(c->feat_grad, rows * 128);
    for (int i = 0; i < a->n_gru; ++i)
        for (int d = 0; d < 2; ++d) { ALLOC(c->dgx[i][d], rows * 384); ALLOC(c->dgh[i][d], rows * 384); }
    // the side stream's slabs: one 384 x 384 product over gemm_tn_max_splits() splits, or a GRU layer's four 128 x 384 ones
    ALLOC(c->tn_slab_side, (size_t)gemm_tn_max_splits() * std::max<size_t>(384 * 384 + 384, 4 * (128 * 384 + 384)));
    // lowest priority: the side stream only carries work nobody waits for soon (weight-gradient GEMMs, the patch Gram
    // matrix); whenever the main stream has a kernel ready it should get the CUs
    int prio_lo = 0, prio_hi = 0;
    hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    // the events only order work between streams of THIS device: no system-scope fence on record (it cost ~4 us of main-stream
    // bubble per fork); host reads go through hipStreamSynchronize, peers through RCCL kernels that run on this device
    if (hipStreamCreateWithPriority(&c->side, hipStreamNonBlocking, prio_lo) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming | hipEventDisableSystemFence) != hipSuccess ||
        // ev_join and the bucket events cross to a caller's communication stream (RCCL reads the gradients there and writes
        // them to peers): they keep the default system-scope release
        hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess ||
        // ev_prep carries DATA from the side stream to the main stream and is waited for microseconds after its record: it keeps the default release, to be on
        // the safe side of DESIGN.md section 6 item 8 (ev_gram, the other side -> main data event, is waited for a millisecond after its record)
        hipEventCreateWithFlags(&c->ev_prep, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_gram, hipEventDisableTiming | hipEventDisableSystemFence) != hipSuccess) {
        seld_destroy(c);
        return fail(nullptr, SELD_ERR_HIP, "side stream / event creation failed");
    }
    for (int i = 0; i < a->n_gru; ++i)
        if (hipEventCreateWithFlags(&c->ev_bucket[i], hipEventDisableTiming) != hipSuccess) {
            seld_destroy(c);
            return fail(nullptr, SELD_ERR_HIP, "event creation failed");
        }
    ALLOC(c->sync_buf, (resn ? 16 * 128 : 128) + 1);      // + this rank's element count, all-reduced with the sums
    for (int hd = 0; hd < 2; ++hd)
        for (auto& D : c->heads[hd].layers) {
            ALLOC(D.y, rows * (size_t)D.out); ALLOC(D.dy, rows * (size_t)D.out);
            if (D.ks > 1) ALLOC(D.xe, rows * (size_t)D.in);
            if (D.rate > 0.f) ALLOC(D.yd, rows * (size_t)D.out);
        }
    {
        size_t tmp = 0;
        for (int hd = 0; hd < 2; ++hd) for (auto& D : c->heads[hd].layers) if (D.ks > 1) tmp = std::max(tmp, rows * (size_t)D.in);
        if (tmp) ALLOC(c->head_tmp, tmp);
        if (a->output_coupling) ALLOC(c->doa_v1, rows * (size_t)(3 * a->n_classes));
    }
    {
        // pre-split bf16 planes: every GRU kernel and the heads' first layers, in the forward ([n][k]) and the
        // input-gradient ([in][out]) orientation
        size_t ne = 0;
        for (int i = 0; i < a->n_gru; ++i) ne += 4 * gemm_sb_split_elems(c->gru[i].in_feat, 384);
        for (int hd = 0; hd < 2; ++hd) ne += 2 * gemm_sb_split_elems(c->heads[hd].layers[0].in, c->heads[hd].layers[0].out);
        ALLOC(c->gsplit, ne);
        unsigned short* q = c->gsplit;
        for (int i = 0; i < a->n_gru; ++i)
            for (int d = 0; d < 2; ++d) {
                c->ksp_fwd[i][d] = q; q += gemm_sb_split_elems(c->gru[i].in_feat, 384);
                c->ksp_bwd[i][d] = q; q += gemm_sb_split_elems(c->gru[i].in_feat, 384);
            }
        for (int hd = 0; hd < 2; ++hd) {
            const DenseL& D = c->heads[hd].layers[0];
            c->h0sp_fwd[hd] = q; q += gemm_sb_split_elems(D.in, D.out);
            c->h0sp_bwd[hd] = q; q += gemm_sb_split_elems(D.in, D.out);
        }
    }
    {
        const int nt = c->heads[0].layers.back().out + c->heads[1].layers.back().out, k = c->heads[0].layers[0].in;
        ALLOC(c->weff, (size_t)(k + 1) * nt);
        ALLOC(c->dy_all, rows * (size_t)nt);
        ALLOC(c->headF, (size_t)k * nt + nt);
    }
    ALLOC(c->loss_scratch, (size_t)loss_scratch_floats((int)rows));
    ALLOC(c->den_dev, 4); ALLOC(c->loss_out, rows + 4);
#undef ALLOC
    { int rc_ = v2_tables_create(c); if (rc_) { g_create_err = c->err; seld_destroy(c); return rc_; } }
    if (hipDeviceSynchronize() != hipSuccess) { seld_destroy(c); return fail(nullptr, SELD_ERR_HIP, "device sync after allocation failed"); }
    *out = c;
    return SELD_OK;
}

void seld_destroy(seld_ctx* c) {
    if (!c) return;
    hipSetDevice(c->device);
    hipDeviceSynchronize();
    for (auto& t : c->timers) for (auto e : t.ev) hipEventDestroy(e);
    for (auto e : c->ev_pool) hipEventDestroy(e);
    if (c->ev_fork) hipEventDestroy(c->ev_fork);
    if (c->ev_join) hipEventDestroy(c->ev_join);
    if (c->ev_prep) hipEventDestroy(c->ev_prep);
    if (c->ev_gram) hipEventDestroy(c->ev_gram);
    if (c->ev_rn_ready) hipEventDestroy(c->ev_rn_ready);
    for (auto e_ : c->ev_rn_free) if (e_) hipEventDestroy(e_);
    for (auto e : c->ev_bucket) if (e) hipEventDestroy(e);
    seld_dp_destroy(c);
    if (c->side) hipStreamDestroy(c->side);
    for (void* p : c->allocs) hipFree(p);
    delete c;
}

int seld_set_stream(seld_ctx* c, void* s) { if (!c) return SELD_ERR_INVALID; c->stream = (hipStream_t)s; return SELD_OK; }
int seld_set_batch(seld_ctx* c, int B) {
    if (!c) return SELD_ERR_INVALID;
    if (B < 1 || B > c->Bmax) return fail(c, SELD_ERR_INVALID, "batch exceeds the size given to seld_create");
    c->B = B;
    return SELD_OK;
}
int seld_set_option(seld_ctx* c, const char* key, int value) {
    if (!c || !key) return SELD_ERR_INVALID;
    if (!strcmp(key, "conv64_split_bf16")) { c->conv64_split_bf16 = value != 0; return SELD_OK; }
    if (!strcmp(key, "gemm_split_bf16")) { c->gemm_split_bf16 = value != 0; return SELD_OK; }
    if (!strcmp(key, "heads_fused")) { c->heads_fused = value != 0; return SELD_OK; }
    if (!strcmp(key, "dropout_seed")) { c->dropout_seed = 0x5e1d5e1d00000000ull ^ (uint64_t)(unsigned)value; return SELD_OK; }      // the masks are a function of (seed, step, layer, element)
    if (!strcmp(key, "dropout_step")) { c->dropout_step = (unsigned)value; return SELD_OK; }                                         // the NEXT training forward's step counter
    if (!strcmp(key, "conv1_split_bf16")) { c->conv1_split_bf16 = value != 0; return SELD_OK; }
    if (!strcmp(key, "gram_bg_blocks") && value >= 16 && value <= 512) { c->kc.gram_bg_blocks = value; return SELD_OK; }   // tuning knob
    if (!strcmp(key, "conv1_pool_fused")) { c->conv1_pool_fused = value != 0; return SELD_OK; }
    if (!strcmp(key, "conv1_gram")) { c->conv1_gram = value != 0; return SELD_OK; }
    if (!strcmp(key, "gru_wgrad_batch")) { c->gru_wgrad_batch = value != 0; return SELD_OK; }
    if (!strcmp(key, "conv2_pre_fused")) { c->conv2_pre_fused = value != 0; return SELD_OK; }
    if (!strcmp(key, "conv3_pre_fused")) { c->conv3_pre_fused = value != 0; return SELD_OK; }
    if (!strcmp(key, "gram_parts") && (value == 1 || value == 2)) { c->gram_parts = value; return SELD_OK; }
    if (!strcmp(key, "xc_fused_fwd")) { c->xc_fused_fwd = value != 0; return SELD_OK; }
    if (!strcmp(key, "rn_split_bf16")) { c->rn_split_bf16 = value != 0; return SELD_OK; }
    if (!strcmp(key, "rn_wgrad_side")) { c->rn_wgrad_side = value != 0; return SELD_OK; }
    if (!strcmp(key, "rn_implicit3x3")) { c->rn_implicit3x3 = value != 0; return SELD_OK; }
    if (!strcmp(key, "rn_epi_stats")) { c->rn_epi_stats = value != 0; return SELD_OK; }
    if (!strcmp(key, "rn_epi_add")) { c->rn_epi_add = value != 0; return SELD_OK; }
    if (!strcmp(key, "xc_wgrad_side")) { c->xc_wgrad_side = value != 0; return SELD_OK; }
    if (!strcmp(key, "xc_fused_pw_bwd")) { c->xc_fused_pw_bwd = value != 0; return SELD_OK; }
    // the context's kernel choices (common.h KernelChoices): its passes hand c->kc to every launcher that chooses by one
    if (!strcmp(key, "bwd_four_products")) { c->kc.bwd_four = value != 0; return SELD_OK; }
    if (!strcmp(key, "tn_tile_blocks") && value >= 64 && value <= 4096) { c->kc.tn_tile_blocks = value; return SELD_OK; }     // gemm_tn_sb.hip
    if (!strcmp(key, "conv_wgrad_side")) { c->conv_wgrad_side = value != 0; return SELD_OK; }
    if (!strcmp(key, "dgrad_r8")) { c->kc.dgrad_r8 = value != 0; return SELD_OK; }
    if (!strcmp(key, "conv1_pingpong")) { c->kc.conv1_pingpong = value != 0; return SELD_OK; }
    if (!strcmp(key, "prep_side")) { c->prep_side = value != 0; return SELD_OK; }
    if (!strcmp(key, "xc_nowait")) { c->xc_nowait = value != 0; return SELD_OK; }
    if (!strcmp(key, "xc_fused_bn_sums")) { c->xc_fused_bn_sums = value != 0; return SELD_OK; }
    if (!strcmp(key, "xc_fused_dw_bwd")) { c->xc_fused_dw_bwd = value != 0; return SELD_OK; }
    if (!strcmp(key, "xc_w16")) { c->kc.xc_w16 = value != 0; return SELD_OK; }               // xception.hip
    if (!strcmp(key, "xc_xcd_map")) { c->kc.xc_xcd_map = value != 0; return SELD_OK; }       // xception.hip
    if (!strcmp(key, "bf16_single")) { c->kc.mfma_one = value != 0; return SELD_OK; }     // = SELD_DTYPE_BF16 at seld_create
    return fail(c, SELD_ERR_INVALID, std::string("unknown option: ") + key);
}
int seld_sync(seld_ctx* c) {
    if (!c) return SELD_ERR_INVALID;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SELD_OK;
}

int64_t seld_param_count(const seld_ctx* c) { return c ? c->nparam : -1; }
int64_t seld_state_count(const seld_ctx* c) { return c ? c->nstate : -1; }
int seld_variable_count(const seld_ctx* c, int trainable) { return c ? (int)(trainable ? c->tr.size() : c->nt.size()) : -1; }
int seld_variable_info(const seld_ctx* c, int trainable, int index, char* name, int name_cap, int64_t* offset,
                       int32_t* rank, int64_t shape[4]) {
    if (!c) return SELD_ERR_INVALID;
    const std::vector<Var>& v = trainable ? c->tr : c->nt;
    if (index < 0 || index >= (int)v.size()) return SELD_ERR_INVALID;
    if (name && name_cap > 0) { strncpy(name, v[index].name.c_str(), name_cap - 1); name[name_cap - 1] = 0; }
    if (offset) *offset = v[index].off;
    if (rank) *rank = v[index].rank;
    if (shape) for (int k = 0; k < 4; ++k) shape[k] = v[index].shape[k];
    return SELD_OK;
}

static int copy_h2d(seld_ctx* c, float* dst, const float* src, int64_t n, int64_t expect) {
    if (!c || !src || n != expect) return fail(c, SELD_ERR_INVALID, "size mismatch in host->device copy");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(dst, src, (size_t)n * 4, hipMemcpyHostToDevice));
    return SELD_OK;
}
static int copy_d2h(seld_ctx* c, float* dst, const float* src, int64_t n, int64_t expect) {
    if (!c || !dst || n != expect) return fail(c, SELD_ERR_INVALID, "size mismatch in device->host copy");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(dst, src, (size_t)n * 4, hipMemcpyDeviceToHost));
    return SELD_OK;
}
int seld_set_weights_host(seld_ctx* c, const float* w, int64_t n) { return c ? copy_h2d(c, c->params, w, n, c->nparam) : SELD_ERR_INVALID; }
int seld_get_weights_host(seld_ctx* c, float* w, int64_t n) { return c ? copy_d2h(c, w, c->params, n, c->nparam) : SELD_ERR_INVALID; }
int seld_set_state_host(seld_ctx* c, const float* s, int64_t n) { return c ? copy_h2d(c, c->state, s, n, c->nstate) : SELD_ERR_INVALID; }
int seld_get_state_host(seld_ctx* c, float* s, int64_t n) { return c ? copy_d2h(c, s, c->state, n, c->nstate) : SELD_ERR_INVALID; }
int seld_get_grads_host(seld_ctx* c, float* g, int64_t n) { return c ? copy_d2h(c, g, c->grads, n, c->nparam) : SELD_ERR_INVALID; }
int seld_get_adam_host(seld_ctx* c, float* m, float* v, int64_t n) {
    if (!c) return SELD_ERR_INVALID;
    int rc = copy_d2h(c, m, c->adam_m, n, c->nparam);
    if (rc) return rc;
    return copy_d2h(c, v, c->adam_v, n, c->nparam);
}
int seld_set_adam_host(seld_ctx* c, const float* m, const float* v, int64_t n, int64_t step) {
    if (!c || step < 0) return SELD_ERR_INVALID;
    int rc = copy_h2d(c, c->adam_m, m, n, c->nparam);
    if (rc) return rc;
    rc = copy_h2d(c, c->adam_v, v, n, c->nparam);
    if (rc) return rc;
    c->adam_step = step;
    return SELD_OK;
}
void* seld_param_ptr(seld_ctx* c) { return c ? c->params : nullptr; }
void* seld_grad_ptr(seld_ctx* c) { return c ? c->grads : nullptr; }

int seld_forward(seld_ctx* c, const float* x, float* sed, float* doa, int training) {
    if (!c || !x) return SELD_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    return forward_impl(c, x, sed, doa, training, false);
}

static int run_losses(seld_ctx* c, const float* y_sed, const float* y_doa, const seld_loss_cfg* cfg, float* sloss,
                      float* dloss, bool want_grads, bool defer_finalize = false) {
    hipStream_t st = c->stream;
    const int rows = c->B * c->S, nc = c->arch.n_classes;
    if (cfg->doa_loss < SELD_DOA_MSE || cfg->doa_loss > SELD_DOA_MSLE) return fail(c, SELD_ERR_INVALID, "bad doa_loss");
    if (cfg->doa_loss == SELD_DOA_MMSE) {
        if (cfg->mmse_den > 0.f) {
            if (hipMemcpyAsync(c->den_dev, &cfg->mmse_den, 4, hipMemcpyHostToDevice, st) != hipSuccess)
                return fail(c, SELD_ERR_HIP, "den copy failed");
            hipStreamSynchronize(st);  // cfg may live on the caller's stack
        } else {
            launch_mmse_den(st, y_doa, c->den_dev, c->loss_scratch, rows, nc);
            // data parallel (seld_dp_init): the mask count of the GLOBAL batch, summed in place on this stream — no host round trip
            // TRAINING path only (want_grads): seld_test_step is not a collective — train.teststep knows nothing about process groups, a
            // validation loop may run on one rank or with unequal batch counts, and its loss is this rank's own num / den
            if (want_grads && c->dp_comm && c->dp_world > 1 && dp_allreduce(c, c->den_dev, 1, SELD_DTYPE_F32, st)) return fail(c, SELD_ERR_HIP, "RCCL all-reduce of the MMSE denominator failed");
        }
    }
    float* sl = sloss ? sloss : c->loss_out;
    float* dl = dloss ? dloss : c->loss_out + 4;
    // fused linear heads: both pre-activation gradients side by side in one [rows][n_sed + n_doa] buffer (the K axis of dfeat)
    const bool lin = heads_lin(c);
    const int n0 = c->heads[0].layers.back().out, nt = n0 + c->heads[1].layers.back().out;
    launch_losses(st, c->heads[0].layers.back().y, c->arch.output_coupling ? c->doa_v1 : c->heads[1].layers.back().y, y_sed, y_doa, cfg->doa_loss, cfg->w_sed,
                  cfg->w_doa, cfg->sed_grad_scale, c->den_dev, sl, dl,
                  want_grads ? (lin ? c->dy_all : c->heads[0].layers.back().dy) : nullptr,
                  want_grads ? (lin ? c->dy_all + n0 : c->heads[1].layers.back().dy) : nullptr, c->loss_scratch, c->B, c->S, nc,
                  lin ? nt : 0, lin ? nt : 0, defer_finalize ? 1 : 0);
    // seldnet_v1: the losses left d / d(doa sed) in the DOA slot; through the product to the two heads' pre-activations
    if (want_grads && c->arch.output_coupling)
        launch_v1_couple_bwd(st, c->heads[0].layers.back().y, c->heads[1].layers.back().y, lin ? c->dy_all : c->heads[0].layers.back().dy,
                             lin ? nt : n0, lin ? c->dy_all + n0 : c->heads[1].layers.back().dy, lin ? nt : nt - n0, rows, nc);
    if (defer_finalize) { c->fin_sl = sl; c->fin_dl = dl; c->fin_doa_loss = cfg->doa_loss; }
    return check_launch(c, "losses");
}

int seld_mmse_den(seld_ctx* c, const float* y_doa, float* den) {
    if (!c || !y_doa || !den) return SELD_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    launch_mmse_den(c->stream, y_doa, den, c->loss_scratch, c->B * c->S, c->arch.n_classes);
    return check_launch(c, "mmse_den");
}

int seld_test_step(seld_ctx* c, const float* x, const float* y_sed, const float* y_doa, const seld_loss_cfg* cfg,
                   float* sed, float* doa, float* sloss, float* dloss) {
    if (!c || !x || !y_sed || !y_doa || !cfg) return SELD_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = forward_impl(c, x, sed, doa, 0, false);
    if (rc) return rc;
    return run_losses(c, y_sed, y_doa, cfg, sloss, dloss, false);
}

int seld_train_fwd_bwd(seld_ctx* c, const float* x, const float* y_sed, const float* y_doa, const seld_loss_cfg* cfg,
                       float* sed, float* doa, float* sloss, float* dloss) {
    if (!c || !x || !y_sed || !y_doa || !cfg) return SELD_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = forward_impl(c, x, sed, doa, 1, true);
    if (rc) return rc;
    // the scalar loss values are finalized on the side stream at the end of the backward pass: nothing in it waits for them
    rc = run_losses(c, y_sed, y_doa, cfg, sloss, dloss, true, true);
    if (rc) return rc;
    return backward_impl(c, x);
}

int seld_adam_step(seld_ctx* c, float lr, float beta1, float beta2, float eps, int agc) {
    if (!c) return SELD_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    if (agc)
        for (auto& v : c->tr) launch_agc(c->stream, c->params, c->grads, v.off, v.rank, v.shape, nullptr);
    c->adam_step += 1;
    const double t = (double)c->adam_step;
    const float lr_t = (float)((double)lr * sqrt(1.0 - pow((double)beta2, t)) / (1.0 - pow((double)beta1, t)));
    PROF2(c, "adam");
    launch_adam(c->stream, c->params, c->grads, c->adam_m, c->adam_v, c->nparam, lr_t, beta1, beta2, eps);
    return check_launch(c, "adam");
}

int seld_train_step(seld_ctx* c, const float* x, const float* y_sed, const float* y_doa, const seld_loss_cfg* cfg,
                    float lr, int agc, float* sed, float* doa, float* sloss, float* dloss) {
    int rc = seld_train_fwd_bwd(c, x, y_sed, y_doa, cfg, sed, doa, sloss, dloss);
    if (rc) return rc;
    return seld_adam_step(c, lr, 0.9f, 0.999f, 1e-7f, agc);
}

// ---------------------------------------------------------------------------------------------- test aid
int seld_debug_pool_routing(seld_ctx* c, int block, unsigned char* pos, unsigned char* gate) {
    if (c && pos && gate && c->arch.first_kind == SELD_FIRST_XCEPTION && block == (int)c->conv.size()) {      // the exit pool of xception_block
        HIPCHK(c, hipSetDevice(c->device));
        if (launch_pool_routing(c->stream, c->xc_x.back(), c->xc_feat, nullptr, c->xc_ident + 128, c->xc_ident + 192, pos, gate, c->B, c->S, 16, 1, 8))
            return fail(c, SELD_ERR_UNSUPPORTED, "pool_routing");
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return check_launch(c, "pool_routing");
    }
    if (!c || !pos || !gate || block < 0 || block >= (int)c->conv.size()) return SELD_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    const ConvL& L = c->conv[block];
    // the first block routes by the positions its forward recorded (with or without the pre-BN tensor); the others by the
    // scan bn_pool_bwd_dz repeats over the stored pre-BN tensor
    const bool recorded = block == 0 && L.amax && (c->gram_active || (L.pf == 4 && (L.pt == 5 || L.pt == 4 || L.pt == 2 || L.pt == 1)));
    if (launch_pool_routing(c->stream, L.z, L.p, recorded ? L.amax : nullptr, L.scale, L.shift, pos, gate, c->B, L.H, L.W, L.pt, L.pf))
        return fail(c, SELD_ERR_UNSUPPORTED, "pool_routing");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return check_launch(c, "pool_routing");
}

static int set_override(seld_ctx* c, int kind, int block, int which, int64_t n, const int64_t* idx_host, const unsigned char* val_host, int64_t limit) {
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < c->overrides.size();)      // replace an earlier list for the same decision tensor (its buffers stay with the ctx)
        if (c->overrides[i].kind == kind && c->overrides[i].block == block && c->overrides[i].which == which) c->overrides.erase(c->overrides.begin() + i);
        else ++i;
    if (n <= 0) return SELD_OK;
    if (!idx_host || !val_host) return SELD_ERR_INVALID;
    for (int64_t k = 0; k < n; ++k)
        if (idx_host[k] < 0 || idx_host[k] >= limit) return fail(c, SELD_ERR_INVALID, "injected decision index out of range");
    seld_ctx::Override o{kind, block, which, n, nullptr, nullptr};
    if (dalloc(c, &o.idx, (size_t)n) || dalloc(c, &o.val, (size_t)n)) return SELD_ERR_NOMEM;
    HIPCHK(c, hipMemcpy(o.idx, idx_host, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(o.val, val_host, (size_t)n, hipMemcpyHostToDevice));
    c->overrides.push_back(o);
    return SELD_OK;
}

int seld_debug_set_routing(seld_ctx* c, int block, int64_t n, const int64_t* idx_host, const unsigned char* val_host) {
    if (c && c->arch.first_kind == SELD_FIRST_XCEPTION && block == (int)c->conv.size()) {      // the exit pool of xception_block
        for (int64_t k = 0; k < n && val_host; ++k)
            if (val_host[k] > 8) return fail(c, SELD_ERR_INVALID, "injected routing value exceeds 1 + the window size");
        return set_override(c, 3, block, 0, n, idx_host, val_host, (int64_t)c->Bmax * c->S * 2 * 64);
    }
    if (!c || block < 0 || block >= (int)c->conv.size()) return SELD_ERR_INVALID;
    const ConvL& L = c->conv[block];
    const int64_t limit = (int64_t)c->Bmax * (L.H / L.pt) * (L.W / L.pf) * 64;
    for (int64_t k = 0; k < n && val_host; ++k)
        if (val_host[k] > L.pt * L.pf) return fail(c, SELD_ERR_INVALID, "injected routing value exceeds 1 + the window size");
    return set_override(c, 0, block, 0, n, idx_host, val_host, limit);
}

int seld_debug_set_relu_gates(seld_ctx* c, int block, int which, int64_t n, const int64_t* idx_host, const unsigned char* val_host) {
    if (!c || which < 0 || which > 2) return SELD_ERR_INVALID;
    if (c->arch.first_kind == SELD_FIRST_XCEPTION) {      // block = unit index 3 b + u: the ReLU in front of that unit
        if (block < 0 || block >= (int)c->xc.size() || which != 0) return SELD_ERR_INVALID;
        return set_override(c, 2, block, 0, n, idx_host, val_host, (int64_t)c->Bmax * c->S * 16 * 64);
    }
    if (c->arch.first_kind != SELD_FIRST_RESNET50 || block < 0 || block >= (int)c->rn.size()) return SELD_ERR_INVALID;
    const RnBlock& R = c->rn[block];
    const int64_t limit = (int64_t)c->Bmax * c->S * R.Wout * (which == 2 ? 4 * R.w : R.w);
    return set_override(c, 1, block, which, n, idx_host, val_host, limit);
}

int seld_debug_relu_output(seld_ctx* c, int block, int which, float* dst, int64_t capacity, int64_t* count) {
    if (!c || !dst || !count || which < 0 || which > 2) return SELD_ERR_INVALID;
    if (c->arch.first_kind == SELD_FIRST_XCEPTION) {      // block = unit index: the value whose sign is the gate of the ReLU in front of that unit
        if (block < 0 || block >= (int)c->xc.size() || which != 0) return SELD_ERR_INVALID;
        HIPCHK(c, hipSetDevice(c->device));
        const int64_t n = (int64_t)c->B * c->S * 16 * 64;
        *count = n;
        if (capacity < n) return fail(c, SELD_ERR_INVALID, "seld_debug_relu_output: destination too small");
        const int b = block / 3, u = block % 3;
        const bool fold = c->xc_fused_fwd && u > 0;
        launch_affine_copy(c->stream, u == 0 ? c->xc_x[b] : (fold ? c->xc[block - 1].z : c->xc[block - 1].a), fold ? c->xc[block - 1].scale : nullptr, dst, n, 64);
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return check_launch(c, "relu_output");
    }
    if (c->arch.first_kind != SELD_FIRST_RESNET50 || block < 0 || block >= (int)c->rn.size()) return SELD_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    const RnBlock& R = c->rn[block];
    const int64_t M = (int64_t)c->B * c->S * R.Wout, n = M * (which == 2 ? 4 * R.w : R.w);
    *count = n;
    if (capacity < n) return fail(c, SELD_ERR_INVALID, "seld_debug_relu_output: destination too small");
    const float* src = which == 0 ? R.y0 : (which == 1 ? R.y1 : R.out);
    HIPCHK(c, hipMemcpyAsync(dst, src, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SELD_OK;
}

// ---------------------------------------------------------------------------------------------- profiling
int seld_profile_enable(seld_ctx* c, int on) {
    if (!c) return SELD_ERR_INVALID;
    c->prof = on < 0 ? 0 : (on > 3 ? 3 : on);
    if (c->prof) {      // events for a default bench run of scopes up front; prof_resolve (seld_profile_get / _reset) recycles them
        hipSetDevice(c->device);
        while (c->ev_pool.size() < (c->prof == 1 ? 1024u : (c->prof == 2 ? 8192u : 32768u))) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) break; c->ev_pool.push_back(e); }
    }
    return SELD_OK;
}
int seld_profile_count(const seld_ctx* c) { return c ? (int)c->timers.size() : -1; }
static void prof_resolve(seld_ctx* c) {
    hipStreamSynchronize(c->stream);
    for (auto& t : c->timers) {
        for (size_t i = 0; i + 1 < t.ev.size(); i += 2) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, t.ev[i], t.ev[i + 1]) == hipSuccess) t.ms += ms;
        }
        for (auto e : t.ev) c->ev_pool.push_back(e);     // recycled by the next timed scopes
        t.ev.clear();
    }
}
int seld_profile_get(seld_ctx* c, int index, char* name, int name_cap, int64_t* launches, double* total_ms) {
    if (!c || index < 0 || index >= (int)c->timers.size()) return SELD_ERR_INVALID;
    prof_resolve(c);
    Timer& t = c->timers[index];
    if (name && name_cap > 0) { strncpy(name, t.name.c_str(), name_cap - 1); name[name_cap - 1] = 0; }
    if (launches) *launches = t.launches;
    if (total_ms) *total_ms = t.ms;
    return SELD_OK;
}
int seld_profile_reset(seld_ctx* c) {
    if (!c) return SELD_ERR_INVALID;
    prof_resolve(c);
    c->timers.clear();
    return SELD_OK;
}

}  // extern "C"
