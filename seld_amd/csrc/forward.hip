// forward.hip — the forward pass of a context: the step's weight pre-pass, then one function per stage (conv blocks, xception_block,
// resnet50_block, GRU layers with the background Gram launches, heads), called in that order by forward_impl.
#include "ctx.h"

#include <stdio.h>

static int prepare_heads_weff(seld_ctx* c, hipStream_t st) {
    const float *w1[2], *b1[2], *w2[2], *b2[2];
    int n[2];
    for (int hd = 0; hd < 2; ++hd) {
        const DenseL &L0 = c->heads[hd].layers[0], &L1 = c->heads[hd].layers[1];
        w1[hd] = c->params + L0.w_off; b1[hd] = c->params + L0.b_off; w2[hd] = c->params + L1.w_off; b2[hd] = c->params + L1.b_off;
        n[hd] = L1.out;
    }
    return launch_heads_weff(st, w1, b1, w2, b2, n, c->heads[0].layers[0].in, c->heads[0].layers[0].out, c->weff);
}

// The GEMM weight operands a step pre-splits (gemm_sb.hip's planes; the weights change every step): the GRU input projections and the heads'
// first layer, each with its gradient orientation when a backward follows.  add(w, planes, ldb, transb, K, N) != 0 stops the walk.
template <typename Add>
static int gemm_split_jobs(seld_ctx* c, bool with_grad_orientation, Add add) {
    for (size_t i = 0; i < c->gru.size(); ++i) {
        const GruL& G = c->gru[i];
        if (!gru_sb(c, G)) continue;
        for (int d = 0; d < 2; ++d) {
            if (add(c->params + G.k_off[d], c->ksp_fwd[i][d], 384, 0, G.in_feat, 384)) return -1;     // gx = feat K
            if (with_grad_orientation && add(c->params + G.k_off[d], c->ksp_bwd[i][d], 384, 1, 384, G.in_feat)) return -1;   // din = dgx K^T
        }
    }
    if (heads_sb(c) && !heads_lin(c))
        for (int hd = 0; hd < 2; ++hd) {
            const DenseL& D = c->heads[hd].layers[0];
            if (add(c->params + D.w_off, c->h0sp_fwd[hd], D.out, 0, D.in, D.out)) return -1;
            if (with_grad_orientation && add(c->params + D.w_off, c->h0sp_bwd[hd], D.out, 1, D.out, D.in)) return -1;
        }
    return 0;
}

// launch_gemm_split_b jobs gathered 16 to a launch (the stand-alone kernel: resnet50_block's planes, and the fallback of forward_weight_prep)
struct GemmSplitBatch {
    seld_ctx* c;
    hipStream_t st;
    const float* src[16]; unsigned short* dst[16]; int ldb[16], tb[16], K[16], N[16];
    int n = 0;
    int flush() { const int rc = n ? launch_gemm_split_b(st, c->kc, n, src, dst, ldb, tb, K, N) : 0; n = 0; return rc; }
    int add(const float* w, unsigned short* d, int ld, int transb, int k, int nn) {
        src[n] = w; dst[n] = d; ldb[n] = ld; tb[n] = transb; K[n] = k; N[n] = nn;
        return ++n == 16 ? flush() : 0;
    }
};

static int prepare_gemm_splits(seld_ctx* c, hipStream_t st, bool with_grad_orientation) {
    GemmSplitBatch b{c, st};
    if (gemm_split_jobs(c, with_grad_orientation, [&](const float* w, unsigned short* d, int ld, int transb, int k, int nn) { return b.add(w, d, ld, transb, k, nn); })) return -1;
    return b.flush();
}

// BatchNormalization of a resnet50_block convolution: statistics (training) or moving statistics -> cv.coef
// nbx_have > 0: the convolution's epilogue already left that many [sum | sum of squares] partials in rn_part (Cout = 64)
// part: the partial-sum scratch (default rn_part; the side stream's projection shortcut has its own)
static void rn_bn(seld_ctx* c, hipStream_t st, RnConv& cv, int64_t M, int training, int nbx_have = 0, float* part = nullptr) {
    int nbx = nbx_have;
    if (!part) part = c->rn_part;
    if (training && !nbx_have) launch_rn_bn_stats(st, cv.z, part, &nbx, M, cv.Cout);
    float *g = c->params + cv.g_off, *be = c->params + cv.be_off, *mm = c->state + cv.mm_off, *mv = c->state + cv.mv_off;
    if (training && c->sync_fn) {
        // synchronised BatchNorm: this rank's per-chunk sums -> the host's all-reduce -> coefficients of the GLOBAL batch
        const int nd = (cv.Cout + 63) / 64 * 128;
        launch_rn_bn_finalize(st, part, nbx, (double)M, g, be, mm, mv, cv.coef, cv.Cout, 1, c->sync_buf, 1);
        if (c->sync_fn(c->sync_user, c->sync_buf, nd + 1, SELD_DTYPE_F64, st)) { c->sync_failed = true; return; }      // + the element count
        launch_rn_bn_finalize(st, part, nbx, 0.0, g, be, mm, mv, cv.coef, cv.Cout, 1, c->sync_buf, 2);
        return;
    }
    launch_rn_bn_finalize(st, part, nbx, (double)M, g, be, mm, mv, cv.coef, cv.Cout, training);
}

// models.seldnet_v1 (models.py:36-52): doa <- tanh(doa * [sed | sed | sed]) after the two heads; the plain model returns as it is
static int heads_couple(seld_ctx* c, float* doa, int rows) {
    if (c->arch.output_coupling)
        launch_v1_couple_fwd(c->stream, c->heads[0].layers.back().y, c->heads[1].layers.back().y, c->doa_v1, doa, rows, c->arch.n_classes);
    return check_launch(c, "forward");
}

// resnet50_block: this step's pre-split weight planes (16 operands per launch), on `st`.  They depend on the parameters only: with `prep_side` they are made
// on the side stream beside the entry convolution and taken back (ev_prep) in front of the first stage (round 5: 0.15 ms of the 14.4-ms step).
static void rn_weight_prep(seld_ctx* c, hipStream_t st, bool save) {
    GemmSplitBatch sb{c, st};
    auto add = [&](const float* w, unsigned short* d, int ld, int transb, int k, int nn) { sb.add(w, d, ld, transb, k, nn); };
    for (auto& R : c->rn)
        for (RnConv* cv : {&R.c[0], &R.c[1], &R.c[2], &R.sc}) {
            const int K = cv->k * cv->k * cv->Cin, N = cv->Cout;
            if (cv->wsp) add(c->params + cv->w_off, cv->wsp, N, 0, K, N);
            if (cv->wsp_t && save) {
                if (cv == &R.c[1] && rn_c1_implicit(c, R)) add(c->params + cv->w_off, cv->wsp_t, N, 2, 9 * N, cv->Cin);    // flipped taps
                else add(c->params + cv->w_off, cv->wsp_t, N, 1, N, K);
            }
        }
    sb.flush();
    const float* w9[8]; unsigned short* d9[8]; int f9[8];
    int n = 0;
    for (auto& R : c->rn) {
        if (!rn_c1_direct(R)) continue;
        const float* wsrc = c->params + R.c[1].w_off;
        if (R.c[1].w2) { launch_rn_w32_embed(st, wsrc, R.c[1].w2); wsrc = R.c[1].w2; }
        w9[n] = wsrc; d9[n] = R.c[1].wsp9; f9[n++] = 0;
        if (save) { w9[n] = wsrc; d9[n] = R.c[1].wsp9_flip; f9[n++] = 1; }
        if (n >= 7) { launch_split_weights_batch(st, c->kc, n, w9, d9, f9); n = 0; }
    }
    if (n) launch_split_weights_batch(st, c->kc, n, w9, d9, f9);
}

// BatchNormalization coefficients of a 64-channel layer (a conv block or an xception unit: the same field names) from `np` partial
// [sum z | sum z^2] rows over `count` elements.  Training: the batch statistics (and the moving statistics' update) — with synchronised
// BatchNorm this rank's sums -> the host's all-reduce -> coefficients of the GLOBAL batch; inference: the moving statistics.
template <typename Layer>
static int bn_coeffs(seld_ctx* c, hipStream_t st, int training, const float* part, int np, double count, Layer& L) {
    const float *g = c->params + L.g_off, *be = c->params + L.be_off;
    float *mm = c->state + L.mm_off, *mv = c->state + L.mv_off;
    if (training && c->sync_fn) {
        launch_bn_partials_to_sums(st, part, np, c->sync_buf, count);
        if (c->sync_fn(c->sync_user, c->sync_buf, 129, SELD_DTYPE_F64, st)) return fail(c, SELD_ERR_HIP, "sync_bn all-reduce callback failed");
        launch_bn_finalize_sums(st, c->sync_buf, 0.0 /* the all-reduced count */, g, be, mm, mv, L.mean, L.invstd, L.scale, L.shift);
    } else if (training)
        launch_bn_finalize(st, part, np, count, g, be, mm, mv, L.mean, L.invstd, L.scale, L.shift, 64, 1);
    else
        launch_bn_eval_coeffs(st, g, be, mm, mv, L.scale, L.shift, 64);
    return SELD_OK;
}

// What one forward pass fixes at its start and every stage reads; lives on forward_impl's stack.  What a stage hands to the next one
// (the feature pointer, where the weight pre-pass ran) is in the stage functions' signatures.
struct FwdPass {
    const float* x;              // the input features: the first conv block, and the Gram launches under the GRU recurrences
    int training;
    bool save;                   // a backward pass follows: keep what it reads
    bool conv_drop, gru_drop;    // training with seld_arch.conv_dropout / gru_dropout > 0
};

// The step's weight pre-pass.  *prep_on_side / *rn_prep_on_side: it went to the side stream and ev_prep marks its end — the conv blocks
// (behind the first block's convolution) / the resnet50_block stages take it back.
static int forward_weight_prep(seld_ctx* c, bool save, bool* prep_on_side, bool* rn_prep_on_side) {
    hipStream_t st = c->stream;
    *prep_on_side = false;
    *rn_prep_on_side = !c->rn.empty() && c->rn_split_bf16 && c->prep_side && c->ev_prep;
    if (*rn_prep_on_side) { fork_side(c); rn_weight_prep(c, c->side, save); hipEventRecord(c->ev_prep, c->side); }
    // every weight-only pre-pass of the step in ONE launch (prep.hip): the split-bf16 planes of the GEMM and 64 -> 64 conv
    // weights (with the gradient orientations / flipped taps when a backward follows) and the folded head weights
    GemmSplitJobs a; SplitWeightJobs b; HeadsLin h;
    int na = 0, nb = 0;
    bool fits = true;
    gemm_split_jobs(c, save, [&](const float* w, unsigned short* d, int ld, int transb, int k, int nn) {
        if (na == GSB_MAX_JOBS) { fits = false; return 1; }
        a.src[na] = w; a.dst[na] = d; a.ldb[na] = ld; a.transb[na] = transb; a.K[na] = k; a.N[na] = nn; ++na;
        return 0;
    });
    a.njobs = na;
    // the 64 -> 64 conv blocks' planes (forward, and flipped taps when a backward follows): one list for either form below
    static_assert(2 * (SELD_MAX_LAYERS - 1) <= 8, "the conv64 weight planes of a step fit one SplitWeightJobs");
    if (c->conv64_split_bf16)
        for (size_t i = 1; i < c->conv.size(); ++i) {
            b.w[nb] = c->params + c->conv[i].w_off; b.dst[nb] = c->wsp_fwd[i]; b.flip[nb++] = 0;
            if (save) { b.w[nb] = c->params + c->conv[i].w_off; b.dst[nb] = c->wsp_bwd[i]; b.flip[nb++] = 1; }
        }
    const bool lin = heads_lin(c);
    if (lin)
        for (int hd = 0; hd < 2; ++hd) {
            const DenseL &L0 = c->heads[hd].layers[0], &L1 = c->heads[hd].layers[1];
            h.w1[hd] = c->params + L0.w_off; h.b1[hd] = c->params + L0.b_off; h.w2[hd] = c->params + L1.w_off;
            h.b2[hd] = c->params + L1.b_off; h.n[hd] = L1.out;
            h.K = L0.in; h.Hd = L0.out;
        }
    if (fits && (!lin || h.K + 1 <= 4 * 144)) {
        // prep_side (round 5): none of these planes is read by the FIRST block's forward (it splits its own 7-channel kernel on load), so the pre-pass runs
        // on the side stream beside it; the main stream takes it back (ev_prep) behind the first block's launch.  The side stream's later work of the step
        // (the Gram launches, the kernel gradients) is ordered behind it by the stream itself.
        *prep_on_side = c->prep_side && c->ev_prep && c->xc.empty() && c->rn.empty() && c->conv.size() >= 2;
        if (*prep_on_side) fork_side(c);
        if (launch_weight_prep(*prep_on_side ? c->side : st, c->kc, a, na, b, nb, h, lin ? c->weff : nullptr)) return fail(c, SELD_ERR_UNSUPPORTED, "weight_prep");
        if (*prep_on_side) hipEventRecord(c->ev_prep, c->side);
    } else {      // more jobs than one launch takes (not a seldnet.json shape): the stand-alone kernels
        if (prepare_gemm_splits(c, st, save)) return fail(c, SELD_ERR_UNSUPPORTED, "gemm_split_b");
        if (lin && prepare_heads_weff(c, st)) return fail(c, SELD_ERR_UNSUPPORTED, "heads_weff");
        if (nb && launch_split_weights_batch(st, c->kc, nb, b.w, b.dst, b.flip)) return fail(c, SELD_ERR_UNSUPPORTED, "split_weights");
    }
    return SELD_OK;
}

// the conv blocks (simple_conv_block, or the entry block of the other FIRST kinds) on p.x; *feat = the last block's output
static int forward_conv_blocks(seld_ctx* c, const FwdPass& p, bool prep_on_side, const float** feat) {
    hipStream_t st = c->stream;
    const int B = c->B;
    const float* in = p.x;
    bool pre_pending = false;
    for (size_t i = 0; i < c->conv.size(); ++i) {
        ConvL& L = c->conv[i];
        bool ext_now = false;
        int npart = 0;
        float* stat = p.training ? c->stat_partial : nullptr;
        char tn[32];
        snprintf(tn, sizeof tn, "conv%d_fwd", (int)i + 1);
        // first block with the seldnet.json (5,4) pool: the conv epilogue reduces every pooling window of z
        // (conv_pool.hip), BN+ReLU+MaxPool becomes an elementwise pass over 1/20 of the data, z is stored
        // only when the backward pass will read it
        const bool fused_pool = i == 0 && c->conv1_pool_fused && L.pt == 5 && L.pf == 4 && L.W == 64;
        const bool gram = fused_pool && p.save && c->conv1_gram;      // backward without the pre-BN tensor: z is not stored
        if (i == 0) c->gram_active = gram;
        // the pooled tensor's BatchNorm + ReLU pass folded into the next block's loader (conv_sb.hip PRE): training with the Gram backward (zext kept
        // beside p), and inference (nobody reads p: the extremes go to zext and p is not written at all)
        const bool pre_next = fused_pool && (gram || !p.save) && c->conv2_pre_fused && !p.conv_drop && c->arch.first_kind == SELD_FIRST_SIMPLE_CONV &&
                              i + 1 < c->conv.size() && c->conv64_split_bf16 && !c->kc.mfma_one && conv64_fwd_sb_takes_pre(c->kc, c->conv[i + 1].W);
        if (fused_pool) {
            PROF(c, tn);   // level 1
            if (launch_conv_first_fwd_pool(st, c->kc, in, c->params + L.w_off, c->params + L.b_off, c->params + L.g_off,
                                           (p.save && !gram) ? L.z : nullptr, (gram || pre_next) ? L.zext : L.p, p.save ? L.amax : nullptr, stat,
                                           &npart, B, L.H, L.Cin, c->conv1_split_bf16))
                return fail(c, SELD_ERR_UNSUPPORTED, "conv_first_fwd_pool");
        } else if (i == 0) {
            PROF(c, tn);   // level 1
            if (launch_conv_first_fwd(st, in, c->params + L.w_off, c->params + L.b_off, L.z, stat, &npart, B, L.H, L.Cin))
                return fail(c, SELD_ERR_UNSUPPORTED, "conv_first_fwd");
            if (p.save && L.pf == 4) launch_pool_argext(st, L.z, c->params + L.g_off, L.amax, B, L.H, L.W, L.pt, L.pf);   // for the fused backward
        } else {
            PROF2(c, tn);
            if (c->conv64_split_bf16) {
                // pre_pending: the first block's BatchNorm + ReLU ride in this block's region load (conv_sb.hip PRE), which also writes its pooled tensor
                const ConvL& P = c->conv[i - 1];
                // ext_now (option "conv3_pre_fused"): this block's (1,4) pooling is split the same way — the epilogue keeps every window's extreme of z
                // (EXT), the NEXT block's loader applies BatchNorm + ReLU to them and writes this block's pooled tensor: no pooling pass over z
                ext_now = pre_pending && c->conv3_pre_fused && L.zext && L.W == 16 && L.pt == 1 && L.pf == 4 && !p.conv_drop && i + 1 < c->conv.size() &&
                          c->conv[i + 1].W == 4 && conv64_fwd_sb_takes_pre(c->kc, 4);
                // (inference: the previous block's activated tensor is read by nobody -> not written)
                if (launch_conv64_fwd_sb(st, c->kc, pre_pending ? P.zext : in, c->wsp_fwd[i], c->params + L.b_off, L.z, stat, &npart, B, L.H, L.W,
                                         pre_pending ? P.scale : nullptr, pre_pending ? P.shift : nullptr, (pre_pending && p.save) ? P.p : nullptr,
                                         ext_now ? c->params + L.g_off : nullptr, ext_now ? L.zext : nullptr))
                    return fail(c, SELD_ERR_UNSUPPORTED, "conv64_fwd_sb");
                pre_pending = false;
            } else if (launch_conv64_fwd(st, in, c->params + L.w_off, c->params + L.b_off, L.z, stat, &npart, B, L.H, L.W))
                return fail(c, SELD_ERR_UNSUPPORTED, "conv64_fwd");
        }
        if (i == 0 && prep_on_side) hipStreamWaitEvent(st, c->ev_prep, 0);      // everything behind the first block's convolution may read the pre-split planes
        if (int rc = bn_coeffs(c, st, p.training, c->stat_partial, npart, (double)B * L.H * L.W, L)) return rc;
        snprintf(tn, sizeof tn, "pool%d_fwd", (int)i + 1);
        // options "conv2_pre_fused" / "conv3_pre_fused" (default 1): the pass is folded into the NEXT block's region load (pre_next: the first block's
        // BatchNorm + ReLU over its window extremes; ext_now: the second block's (1,4) pooling, whose extremes its own epilogue kept) — no launch here
        if (pre_next || ext_now)
            pre_pending = true;
        else {
            PROF2(c, tn);
            if (fused_pool)     // elementwise over zext (in place unless the backward keeps zext)
                launch_bn_relu_ext(st, gram ? L.zext : L.p, L.scale, L.shift, L.p, (int64_t)B * (L.H / 5) * 16 * 64);
            else if (launch_bn_relu_pool_fwd(st, L.z, L.scale, L.shift, L.p, B, L.H, L.W, 64, L.pt, L.pf))
                return fail(c, SELD_ERR_UNSUPPORTED, "bn_relu_pool_fwd");
        }
        in = L.p;
        if (p.conv_drop) {      // Dropout behind the pool (stream 64 + i); the backward masks the gradient arriving at this block with the same draws
            launch_dropout(st, L.p, L.pd, (int64_t)B * (L.H / L.pt) * (L.W / L.pf) * 64, c->arch.conv_dropout, c->dropout_seed, 64u + (unsigned)i, c->dropout_cur);
            in = L.pd;
        }
    }
    *feat = in;
    return SELD_OK;
}

// xception_block middle flow + exit (spec/XCEPTION_BLOCK.md) on the entry block's [B,S,16,64] output (xc_x[0]); *feat = the exit pool's output
static int forward_xception(seld_ctx* c, const FwdPass& p, const float** feat) {
    hipStream_t st = c->stream;
    const int B = c->B, S = c->S;
    const int64_t npix = (int64_t)B * S * 16;
    for (size_t i = 0; i < c->xc.size(); ++i) {
        XcUnit& U = c->xc[i];
        const size_t b = i / 3, u = i % 3;
        // with the fused unit kernel the previous unit's BatchNormalization is applied on load (relu(z scale + shift) of ITS pre-BN
        // tensor): units 0 and 1 of a module then never materialise their normalised output
        const bool fold = c->xc_fused_fwd && u > 0;
        const float* uin = u == 0 ? c->xc_x[b] : (fold ? c->xc[i - 1].z : c->xc[i - 1].a);
        const float* aff = fold ? c->xc[i - 1].scale : nullptr;      // [scale 64 | shift 64]
        int np = 0;
        if (c->xc_fused_fwd) {
            // depthwise + pointwise + BatchNorm statistics in one pass over the unit's input (xception.hip: xc_unit_fwd_kernel)
            PROF2(c, "xc_unit_fwd");
            if (launch_xc_unit_fwd(st, uin, c->params + U.dw_off, c->params + U.pw_off, U.dwo, U.z, p.training ? c->xc_part : nullptr, &np, B, S, 16, aff))
                return fail(c, SELD_ERR_UNSUPPORTED, "xc_unit_fwd");
            if (np > xc_partial_capacity()) return fail(c, SELD_ERR_INVALID, "xception_block: more BatchNorm partials than xc_part holds");
        } else {
        {
            PROF2(c, "xc_depthwise_fwd");
            launch_dw3x3_fwd(st, c->kc, uin, c->params + U.dw_off, U.dwo, B, S, 16);       // ReLU on load, no bias
        }
        {
            PROF2(c, "xc_pointwise_fwd");
            launch_gemm(st, U.dwo, 64, c->params + U.pw_off, 64, nullptr, U.z, 64, (int)npix, 64, 64, 0, 0, 0);
        }
        }
        PROF2(c, "xc_bn_fwd");
        if (p.training && !c->xc_fused_fwd) launch_xc_bn_stats(st, U.z, c->xc_part, &np, npix);
        if (int rc = bn_coeffs(c, st, p.training, c->xc_part, np, (double)npix, U)) return rc;
        if (u == 2 || !c->xc_fused_fwd)
            launch_xc_bn_apply(st, U.z, U.scale, U.shift, u == 2 ? c->xc_x[b] : nullptr, u == 2 ? c->xc_x[b + 1] : U.a, npix);
    }
    // exit: ReLU -> MaxPooling2D((1, 8)) = the BN+ReLU+pool kernel with identity coefficients
    PROF2(c, "xc_exit_pool");
    if (launch_bn_relu_pool_fwd(st, c->xc_x.back(), c->xc_ident + 128, c->xc_ident + 192, c->xc_feat, B, S, 16, 64, 1, 8))
        return fail(c, SELD_ERR_UNSUPPORTED, "xception exit pool");
    *feat = c->xc_feat;
    return SELD_OK;
}

// resnet50_block stages (spec/RESNET50_BLOCK.md) on *feat = the entry block's output: every convolution a product (resnet.hip:
// launch_rn_product_*); *feat becomes the last block's output.  rn_prep_on_side: see forward_weight_prep
static int forward_resnet(seld_ctx* c, const FwdPass& p, bool rn_prep_on_side, const float** feat) {
    hipStream_t st = c->stream;
    const int B = c->B, S = c->S;
    PROF(c, "rn_stages_fwd");
    const bool sb = c->rn_split_bf16 != 0;
    const bool epi_stats = p.training && c->rn_epi_stats;      // BatchNorm statistics in the products' epilogues (common.h GemmEpi)
    if (sb) {      // this step's weight planes: made at the start of the forward on the side stream (rn_prep_on_side), or here
        PROF3(c, "rn_weight_prep");
        if (rn_prep_on_side) hipStreamWaitEvent(st, c->ev_prep, 0);
        else rn_weight_prep(c, st, p.save);
    }
    const float* X = *feat;      // [B,S,Win,Cin]
    int rc_ = 0;
    for (auto& R : c->rn) {
        if (c->sync_failed) break;     // a failed SyncBN collective: enqueue nothing further (the error is reported below)
        const int64_t M = (int64_t)B * S * R.Wout;
        const int w = R.w;
        // the projection shortcut (first block of a stage) depends on the block input only: side stream, joined before the add
        const bool sc_side = R.proj && c->rn_wgrad_side && !c->sync_fn;
        if (sc_side) {
            hipEventRecord(c->ev_rn_ready, st); hipStreamWaitEvent(c->side, c->ev_rn_ready, 0);
            int nb_ = 0;
            if (launch_rn_product_fwd(c->side, c->kc, X, R.Cin * R.stride_f, c->params + R.sc.w_off, sb ? R.sc.wsp : nullptr, R.sc.z, (int)M, R.Cin, 4 * w,
                                      epi_stats ? c->rn_part_side : nullptr, &nb_, c->rn_part_floats))
                return fail(c, SELD_ERR_INVALID, "resnet50_block: projection shortcut product refused");
            rn_bn(c, c->side, R.sc, M, p.training, nb_, c->rn_part_side);
            hipEventRecord(c->ev_rn_free[0], c->side);
        }
        // 1x1 (frequency stride = doubled row stride of the operand), BN, ReLU
        int nb0 = 0;
        { PROF3(c, "rn_products_fwd"); rc_ = launch_rn_product_fwd(st, c->kc, X, R.Cin * R.stride_f, c->params + R.c[0].w_off, sb ? R.c[0].wsp : nullptr, R.c[0].z, (int)M, R.Cin, w,
                                                                   epi_stats ? c->rn_part : nullptr, &nb0, c->rn_part_floats); }
        if (rc_) return fail(c, SELD_ERR_INVALID, "resnet50_block: reduce convolution's product refused");
        { PROF3(c, "rn_bn_fwd"); rn_bn(c, st, R.c[0], M, p.training, nb0); }
        { PROF3(c, "rn_bn_fwd"); launch_rn_bn_apply(st, R.c[0].z, R.c[0].coef, nullptr, R.y0, M, w, 1); }
        // 3x3, BN, ReLU: 64 -> 64 (stage 1) on the implicit-GEMM kernel of the conv blocks (BatchNorm's sums from its epilogue),
        // the other widths as a product on im2col rows
        if (sb && rn_c1_direct(R)) {
            int npart = 0;
            if (R.c[1].w2) {      // stage 0: the epilogue's sums are per (bin parity, channel): the statistics pass instead
                { PROF3(c, "rn_products_fwd"); launch_conv64_fwd_sb(st, c->kc, R.y0, R.c[1].wsp9, nullptr, R.c[1].z, nullptr, nullptr, B, S, rn_c1_width(R)); }
                { PROF3(c, "rn_bn_fwd"); rn_bn(c, st, R.c[1], M, p.training); }
            } else {
                // the conv epilogue's partial sums land in rn_part: at most conv_sb_partial_capacity() [128]-float partials, which must fit before the launch
                if (p.training && (size_t)conv_sb_partial_capacity() * 128 > c->rn_part_floats)
                    return fail(c, SELD_ERR_INVALID, "resnet50_block: more BatchNorm partials than rn_part holds");
                { PROF3(c, "rn_products_fwd"); launch_conv64_fwd_sb(st, c->kc, R.y0, R.c[1].wsp9, nullptr, R.c[1].z, p.training ? c->rn_part : nullptr, &npart, B, S, R.Wout); }
                { PROF3(c, "rn_bn_fwd"); rn_bn(c, st, R.c[1], M, p.training, npart); }
            }
        } else if (sb && rn_c1_implicit(c, R)) {
            int nb1 = 0;
            { PROF3(c, "rn_products_fwd"); rc_ = launch_rn_conv3_fwd(st, c->kc, R.y0, R.c[1].wsp, R.c[1].z, B, S, R.Wout, w, w, epi_stats ? c->rn_part : nullptr, &nb1,
                                                                     c->rn_part_floats); }
            if (rc_) return fail(c, SELD_ERR_INVALID, "resnet50_block: 3x3 convolution's product refused");
            { PROF3(c, "rn_bn_fwd"); rn_bn(c, st, R.c[1], M, p.training, nb1); }
        } else {
            // (only with rn_split_bf16 / rn_implicit3x3 off, or a width no direct kernel takes: the col tensor is allocated here, once)
            if (!R.c[1].col && dalloc(c, &R.c[1].col, (size_t)M * 9 * w)) return fail(c, SELD_ERR_NOMEM, "im2col tensor");
            launch_im2col3x3(st, R.y0, R.c[1].col, B, S, R.Wout, w);
            int nb1 = 0;
            { PROF3(c, "rn_products_fwd"); rc_ = launch_rn_product_fwd(st, c->kc, R.c[1].col, 9 * w, c->params + R.c[1].w_off, sb ? R.c[1].wsp : nullptr, R.c[1].z, (int)M, 9 * w, w,
                                                                       epi_stats ? c->rn_part : nullptr, &nb1, c->rn_part_floats); }
            if (rc_) return fail(c, SELD_ERR_INVALID, "resnet50_block: 3x3 convolution's product refused");
            { PROF3(c, "rn_bn_fwd"); rn_bn(c, st, R.c[1], M, p.training, nb1); }
        }
        { PROF3(c, "rn_bn_fwd"); launch_rn_bn_apply(st, R.c[1].z, R.c[1].coef, nullptr, R.y1, M, w, 1); }
        // 1x1 expand, BN; shortcut; out = ReLU(y + r)
        int nb2 = 0;
        { PROF3(c, "rn_products_fwd"); rc_ = launch_rn_product_fwd(st, c->kc, R.y1, w, c->params + R.c[2].w_off, sb ? R.c[2].wsp : nullptr, R.c[2].z, (int)M, w, 4 * w,
                                                                   epi_stats ? c->rn_part : nullptr, &nb2, c->rn_part_floats); }
        if (rc_) return fail(c, SELD_ERR_INVALID, "resnet50_block: expand convolution's product refused");
        { PROF3(c, "rn_bn_fwd"); rn_bn(c, st, R.c[2], M, p.training, nb2); }
        if (R.proj) {
            if (sc_side) hipStreamWaitEvent(st, c->ev_rn_free[0], 0);
            else {
                int nbs = 0;
                { PROF3(c, "rn_products_fwd"); rc_ = launch_rn_product_fwd(st, c->kc, X, R.Cin * R.stride_f, c->params + R.sc.w_off, sb ? R.sc.wsp : nullptr, R.sc.z, (int)M, R.Cin, 4 * w,
                                                                           epi_stats ? c->rn_part : nullptr, &nbs, c->rn_part_floats); }
                if (rc_) return fail(c, SELD_ERR_INVALID, "resnet50_block: projection shortcut product refused");
                { PROF3(c, "rn_bn_fwd"); rn_bn(c, st, R.sc, M, p.training, nbs); }
            }
            { PROF3(c, "rn_bn_fwd"); launch_rn_bn_apply2(st, R.c[2].z, R.c[2].coef, R.sc.z, R.sc.coef, R.out, M, 4 * w, p.save ? R.gate : nullptr); }
        } else {
            { PROF3(c, "rn_bn_fwd"); launch_rn_bn_apply(st, R.c[2].z, R.c[2].coef, X, R.out, M, 4 * w, 1, p.save ? R.gate : nullptr); }
        }
        X = R.out;
    }
    if (c->sync_failed) { c->sync_failed = false; return fail(c, SELD_ERR_HIP, "sync_bn all-reduce callback failed"); }
    *feat = X;       // [B,S,2,1024] = [B,S,2048]
    return SELD_OK;
}

// the bidirectional GRU layers on *feat ([B,S,128]; force_1d_inputs: feature = f*64 + c), the first block's Gram launches (on p.x) under
// their recurrences on the side stream; *feat becomes the last layer's output
static int forward_gru(seld_ctx* c, const FwdPass& p, const float** feat_io) {
    hipStream_t st = c->stream;
    const int B = c->B, S = c->S, rows = B * S;
    const float* feat = *feat_io;
    const int gparts = !c->gram_active ? 0 : (c->gram_parts == 2 && c->gru.size() >= 2 ? 2 : 1);
    int gram_ns = 0;
    for (size_t i = 0; i < c->gru.size(); ++i) {
        GruL& G = c->gru[i];
        if (p.gru_drop) {
            // Keras GRU dropout / recurrent_dropout (modules.py:312-314): each direction's cell draws its own input mask (stream 96 + 4 i + d) and
            // state mask (98 + 4 i + d); the directions no longer share their input rows, so the projections are two products
            PROF(c, "gru_fwd");
            const float rate = c->arch.gru_dropout;
            for (int d = 0; d < 2; ++d) {
                launch_dropout(st, c->ones, G.imask[d], (int64_t)B * G.in_feat, rate, c->dropout_seed, 96u + 4u * (unsigned)i + d, c->dropout_cur);
                launch_dropout(st, c->ones, G.rmask[d], (int64_t)B * 128, rate, c->dropout_seed, 98u + 4u * (unsigned)i + d, c->dropout_cur);
                launch_mask_rows(st, feat, G.imask[d], G.xm[d], rows, S, G.in_feat, 0);
                if (gru_sb(c, G) && gemm_sb_usable(G.xm[d], G.in_feat, 384, G.in_feat))
                    launch_gemm_sb(st, c->kc, false, GemmEpi(), G.xm[d], nullptr, G.in_feat, c->ksp_fwd[i][d], nullptr, c->params + G.b_off[d], nullptr, G.gx[d], nullptr, 384, rows, 384,
                                   G.in_feat, 0, 0);
                else
                    launch_gemm(st, G.xm[d], G.in_feat, c->params + G.k_off[d], 384, c->params + G.b_off[d], G.gx[d], 384, rows, 384, G.in_feat, 0, 0, 0);
            }
            if (launch_gru_fwd(st, G.gx[0], G.gx[1], c->params + G.u_off[0], c->params + G.u_off[1], c->params + G.b_off[0] + 384,
                               c->params + G.b_off[1] + 384, G.h[0], G.h[1], G.sv[0], G.sv[1], B, S, G.rmask[0], G.rmask[1], G.hm[0], G.hm[1]))
                return fail(c, SELD_ERR_UNSUPPORTED, "gru_fwd (dropout)");
        } else {
        {
            PROF2(c, "gru_inproj_gemm");
            // both directions' projections of the same input in one launch
            if (gru_sb(c, G) && gemm_sb_usable(feat, G.in_feat, 384, G.in_feat))
                launch_gemm_sb(st, c->kc, false, GemmEpi(), feat, nullptr, G.in_feat, c->ksp_fwd[i][0], c->ksp_fwd[i][1], c->params + G.b_off[0],
                               c->params + G.b_off[1], G.gx[0], G.gx[1], 384, rows, 384, G.in_feat, 0, 1);
            else
                launch_gemm_dual_n(st, feat, G.in_feat, c->params + G.k_off[0], c->params + G.k_off[1], 384, c->params + G.b_off[0],
                                   c->params + G.b_off[1], G.gx[0], G.gx[1], 384, rows, 384, G.in_feat, 0, 0);
        }
        if ((int)i < gparts) fork_side(c);
        {
            PROF(c, "gru_fwd");
            launch_gru_fwd(st, G.gx[0], G.gx[1], c->params + G.u_off[0], c->params + G.u_off[1], c->params + G.b_off[0] + 384,
                           c->params + G.b_off[1] + 384, G.h[0], G.h[1], p.save ? G.sv[0] : nullptr, p.save ? G.sv[1] : nullptr, B, S);
        }
        }
        if ((int)i < gparts && p.gru_drop) fork_side(c);
        if ((int)i < gparts) {
            // Gram matrix of the input patches (conv_gram.hip): depends on x alone -> side stream, under the GRU
            // recurrences (2B of the 256 CUs): eligible when the first GRU kernel is (fork event recorded in front of it) but
            // enqueued after it, on a lower-priority stream, so that the recurrence gets its CUs first
            // option "gram_parts" = 2: half of the tiles under each of the first two layers' recurrences (each part released by its own fork)
            int ns = 0;
            const int kp = conv_gram_dim(c->conv[0].Cin);
            if (i == 0) gram_ns = 0;
            if (launch_conv_first_gram(c->side, c->kc, p.x, c->gram_slab + (size_t)gram_ns * kp * kp, &ns, B, c->conv[0].H, c->conv[0].Cin, 1, (int)i, gparts))
                return fail(c, SELD_ERR_UNSUPPORTED, "conv_first_gram");
            gram_ns += ns;
            if ((int)i == gparts - 1) {
                launch_reduce_slabs(c->side, c->gram_slab, gram_ns, (int64_t)kp * kp, c->gram, (int64_t)kp * kp, 0);
                hipEventRecord(c->ev_gram, c->side);
            }
        }
        launch_mul(st, G.h[0], G.h[1], G.out, (int64_t)rows * 128);
        feat = G.out;
    }
    *feat_io = feat;
    return SELD_OK;
}

// the two heads on the last GRU layer's output, in one of three forms (heads_lin, heads_general, the layer chain)
static int forward_heads(seld_ctx* c, const FwdPass& p, const float* feat, float* sed, float* doa) {
    hipStream_t st = c->stream;
    const int rows = c->B * c->S;
    {
        PROF2(c, "heads_fwd");
        // the first layers of the two heads read the same features: one launch when their shapes agree (seldnet.json:
        // Conv1D(128) in both) and neither is the head's output layer
        DenseL &S0 = c->heads[0].layers[0], &D0 = c->heads[1].layers[0];
        if (heads_lin(c)) {
            DenseL &S1 = c->heads[0].layers[1], &D1 = c->heads[1].layers[1];
            const int nt = S1.out + D1.out;
            if (launch_gemm_heads(st, feat, S0.in, c->weff, c->weff + (size_t)S0.in * nt, S1.y, D1.y, sed, doa, rows, S1.out, D1.out,
                                  S0.in, c->heads[0].act, c->heads[1].act))
                return fail(c, SELD_ERR_UNSUPPORTED, "gemm_heads");
            return heads_couple(c, doa, rows);
        }
        if (heads_general(c)) {
            // layer by layer: [rows laid side by side ->] product + bias + activation [-> dropout]
            for (int hd = 0; hd < 2; ++hd) {
                const float* a = feat;
                Head& Hd = c->heads[hd];
                float* outp = hd == 0 ? sed : doa;
                for (size_t j = 0; j < Hd.layers.size(); ++j) {
                    DenseL& D = Hd.layers[j];
                    const bool lastl = (j + 1 == Hd.layers.size());
                    if (D.ks > 1) { launch_time_expand(st, a, D.xe, c->B, c->S, D.in_base, D.ks); a = D.xe; }
                    launch_gemm_mirror(st, a, D.in, c->params + D.w_off, D.out, c->params + D.b_off, D.y, lastl ? outp : nullptr, D.out,
                                       rows, D.out, D.in, 0, lastl ? Hd.act : Hd.hidden_act);
                    a = D.y;
                    if (!lastl && D.rate > 0.f && p.training) {
                        launch_dropout(st, D.y, D.yd, (int64_t)rows * D.out, D.rate, c->dropout_seed, D.drop_id, c->dropout_cur);
                        a = D.yd;
                    }
                }
            }
            return heads_couple(c, doa, rows);
        }
        const bool merged0 = c->heads[0].layers.size() > 1 && c->heads[1].layers.size() > 1 && S0.in == D0.in && S0.out == D0.out &&
                             c->heads[0].hidden_act == c->heads[1].hidden_act;      // one launch, one epilogue activation
        const int hact0 = c->heads[0].hidden_act;
        if (merged0 && heads_sb(c) && gemm_sb_usable(feat, S0.in, S0.out, S0.in))
            launch_gemm_sb(st, c->kc, false, GemmEpi(), feat, nullptr, S0.in, c->h0sp_fwd[0], c->h0sp_fwd[1], c->params + S0.b_off, c->params + D0.b_off, S0.y,
                           D0.y, S0.out, rows, S0.out, S0.in, hact0, 1);
        else if (merged0)
            launch_gemm_dual_n(st, feat, S0.in, c->params + S0.w_off, c->params + D0.w_off, S0.out, c->params + S0.b_off,
                               c->params + D0.b_off, S0.y, D0.y, S0.out, rows, S0.out, S0.in, 0, hact0);
        for (int hd = 0; hd < 2; ++hd) {
            const float* a = feat;
            Head& Hd = c->heads[hd];
            float* outp = hd == 0 ? sed : doa;
            for (size_t j = 0; j < Hd.layers.size(); ++j) {
                DenseL& D = Hd.layers[j];
                const bool lastl = (j + 1 == Hd.layers.size());
                float* y = D.y;
                // the head's output layer also writes the caller's copy (no device-to-device copy afterwards)
                if (!(merged0 && j == 0))
                    launch_gemm_mirror(st, a, D.in, c->params + D.w_off, D.out, c->params + D.b_off, y, lastl ? outp : nullptr, D.out,
                                       rows, D.out, D.in, 0, lastl ? Hd.act : Hd.hidden_act);
                a = y;
            }
        }
    }
    return heads_couple(c, doa, rows);
}

int forward_impl(seld_ctx* c, const float* x, float* sed, float* doa, int training, bool save) {
    c->last_training = training;
    if (training) c->dropout_cur = c->dropout_step++;      // every training forward draws new masks (Keras), backward or not
    const FwdPass p = {x, training, save, training && c->arch.conv_dropout > 0.f, training && c->arch.gru_dropout > 0.f};
    if (p.gru_drop && !save) return fail(c, SELD_ERR_UNSUPPORTED, "gru_dropout: a training forward without saved gates");
    bool prep_on_side = false, rn_prep_on_side = false;
    const float* feat = nullptr;
    int rc = forward_weight_prep(c, save, &prep_on_side, &rn_prep_on_side);
    if (!rc) rc = forward_conv_blocks(c, p, prep_on_side, &feat);
    if (!rc && c->arch.first_kind == SELD_FIRST_XCEPTION) rc = forward_xception(c, p, &feat);
    if (!rc && c->arch.first_kind == SELD_FIRST_RESNET50) rc = forward_resnet(c, p, rn_prep_on_side, &feat);
    if (!rc) rc = forward_gru(c, p, &feat);
    if (!rc) rc = forward_heads(c, p, feat, sed, doa);
    return rc;
}
