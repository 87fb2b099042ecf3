// backward.hip — the backward pass of a context, one function per stage in the reverse order of the forward pass (heads, GRU layers,
// resnet50_block, xception_block, conv blocks), called by backward_impl; the weight gradients go to the side stream.
#include "ctx.h"

#include <algorithm>
#include <stdio.h>

// dW[K1,N] = A^T B and db[N] = colsum(B) in one TN launch + one fixed-order slab reduction
static void wgrad_dense(seld_ctx* c, hipStream_t st, float* slab, const float* A, int lda, const float* Bm, int ldb, int M,
                        int K1, int N, int64_t w_off, int64_t b_off, int S, int shift) {
    int ns = 0;
    // both slab buffers hold gemm_tn_max_splits() slabs of 384 x 384 + 384 floats: larger products (a 2048-feature GRU input) take fewer splits
    const int64_t cap = tn_slab_capacity() / ((int64_t)K1 * N + N);
    if (c->gemm_split_bf16 && gemm_tn_sb_usable(A, lda, Bm, ldb, K1, N)) launch_gemm_tn_sb(st, c->kc, A, lda, Bm, ldb, slab, &ns, M, N, S, shift, 1);
    else launch_gemm_tn(st, A, lda, Bm, ldb, slab, &ns, M, K1, N, S, shift, 1, (int)std::min<int64_t>(cap, gemm_tn_max_splits()));
    launch_reduce_slabs2(st, slab, ns, (int64_t)K1 * N + N, c->grads + w_off, (int64_t)K1 * N, c->grads + b_off, N);
}

// backward of a resnet50_block convolution's BatchNormalization (forward.hip rn_bn): dz = BN'(dy [mask > 0]) into `dz`, dgamma / dbeta into the gradient buffer
// gate4 == nullptr: the BatchNorm feeds a ReLU directly (no residual) and the gate is recomputed from z; else the block output's gate bytes
static void rn_bn_bwd(seld_ctx* c, hipStream_t st, RnConv& cv, const float* dy, const unsigned char* gate4, float* dz, int64_t M) {
    int nbx = 0;
    const int gate_z = gate4 ? 2 : 1;
    const float* mask = reinterpret_cast<const float*>(gate4);
    launch_rn_bn_bwd_reduce(st, cv.z, dy, mask, cv.coef, c->rn_part, &nbx, M, cv.Cout, gate_z);
    if (c->sync_fn) {
        const int nd = (cv.Cout + 63) / 64 * 128;
        launch_rn_bn_bwd_finalize(st, c->rn_part, nbx, (double)M, c->grads + cv.g_off, c->grads + cv.be_off, cv.coef, cv.Cout, c->sync_buf, 1);
        if (c->sync_fn(c->sync_user, c->sync_buf, nd + 1, SELD_DTYPE_F64, st)) { c->sync_failed = true; return; }
        launch_rn_bn_bwd_finalize(st, c->rn_part, nbx, 0.0, c->grads + cv.g_off, c->grads + cv.be_off, cv.coef, cv.Cout, c->sync_buf, 2);
    } else
        launch_rn_bn_bwd_finalize(st, c->rn_part, nbx, (double)M, c->grads + cv.g_off, c->grads + cv.be_off, cv.coef, cv.Cout);
    launch_rn_bn_bwd_dz(st, cv.z, dy, mask, cv.coef, dz, M, cv.Cout, gate_z);
}

// weight gradients of the fused linear heads, on the side stream (the caller has forked): F = feat^T dy and colsum(dy) in one TN
// launch, then the four tensors of each head from them
static void heads_lin_side(seld_ctx* c, int rows) {
    const DenseL& S0 = c->heads[0].layers[0];
    const GruL& Glast = c->gru.back();
    const int nt = c->heads[0].layers[1].out + c->heads[1].layers[1].out, K = S0.in;
    int ns = 0;
    launch_gemm_tn(c->side, Glast.out, K, c->dy_all, nt, c->tn_slab_side, &ns, rows, K, nt, 0, 0, 1);
    launch_reduce_slabs2(c->side, c->tn_slab_side, ns, (int64_t)K * nt + nt, c->headF, (int64_t)K * nt, c->headF + (size_t)K * nt, nt);
    const float *w1[2], *b1[2], *w2[2];
    float *dw1[2], *db1[2], *dw2[2], *db2[2];
    int n[2];
    for (int hd = 0; hd < 2; ++hd) {
        const DenseL &L0 = c->heads[hd].layers[0], &L1 = c->heads[hd].layers[1];
        w1[hd] = c->params + L0.w_off; b1[hd] = c->params + L0.b_off; w2[hd] = c->params + L1.w_off;
        dw1[hd] = c->grads + L0.w_off; db1[hd] = c->grads + L0.b_off; dw2[hd] = c->grads + L1.w_off; db2[hd] = c->grads + L1.b_off;
        n[hd] = L1.out;
    }
    launch_heads_grad(c->side, w1, b1, w2, dw1, db1, dw2, db2, n, K, S0.out, c->headF, c->headF + (size_t)K * nt);
}

// test aid: injected routing decisions edit the tensors the backward kernels read their decisions from (the forward is done with them)
static int apply_overrides(seld_ctx* c) {
    hipStream_t st = c->stream;
    for (const auto& o : c->overrides) {
        if (o.kind == 0) {
            ConvL& L = c->conv[o.block];
            const bool recorded = o.block == 0 && L.amax && (c->gram_active || (L.pf == 4 && (L.pt == 5 || L.pt == 4 || L.pt == 2 || L.pt == 1)));
            if (!recorded && !L.z) return fail(c, SELD_ERR_UNSUPPORTED, "seld_debug_set_routing: this block keeps neither recorded positions nor its pre-BN tensor");
            launch_pool_routing_patch(st, L.z, L.p, recorded ? L.amax : nullptr, L.scale, L.shift, o.idx, o.val, o.n, L.H, L.W, L.pt, L.pf);
        } else if (o.kind == 2) {      // xception_block: the ReLU in front of unit o.block's depthwise convolution
            const int b = o.block / 3, u = o.block % 3;
            const bool fold = c->xc_fused_fwd && u > 0;
            if (fold) launch_relu_gate_patch_z(st, c->xc[o.block - 1].z, nullptr, c->xc[o.block - 1].scale, c->xc[o.block - 1].scale + 64, 64, o.idx, o.val, o.n);
            else launch_relu_gate_patch(st, u == 0 ? c->xc_x[b] : c->xc[o.block - 1].a, nullptr, o.idx, o.val, o.n);
        } else if (o.kind == 3) {      // xception_block: the exit's MaxPool(ReLU(.)) over (1, 8), scanned from the last module's output
            launch_pool_routing_patch(st, c->xc_x.back(), c->xc_feat, nullptr, c->xc_ident + 128, c->xc_ident + 192, o.idx, o.val, o.n, c->S, 16, 1, 8);
        } else {
            RnBlock& R = c->rn[o.block];
            if (o.which == 2) launch_relu_gate_patch(st, R.out, R.gate, o.idx, o.val, o.n);      // read from the gate bits (and the output's sign)
            else {      // recomputed by the backward kernels from the pre-BN tensor and the forward's scale / shift (coef + 2C, + 3C)
                RnConv& K = R.c[o.which];
                launch_relu_gate_patch_z(st, K.z, o.which == 0 ? R.y0 : R.y1, K.coef + 2 * K.Cout, K.coef + 3 * K.Cout, K.Cout, o.idx, o.val, o.n);
            }
        }
    }
    return SELD_OK;
}

// heads: the input-gradient chain runs on the main stream and leaves the gradient w.r.t. the last GRU layer's output in c->feat_grad;
// the weight/bias gradients only feed Adam, so they go to the side stream and overlap with the BPTT chain that follows
static int backward_heads(seld_ctx* c) {
    hipStream_t st = c->stream;
    const int rows = c->B * c->S;
    GruL& Glast = c->gru.back();
    PROF2(c, "heads_bwd");
    float* dfeat = c->feat_grad;
    DenseL &S0 = c->heads[0].layers[0], &D0 = c->heads[1].layers[0];
    if (heads_lin(c)) {
        // dfeat = [dy_sed | dy_doa] Weff^T (K = 48), then on the side stream F = feat^T dy, colsum(dy) and the four
        // gradients of each head from them
        const int nt = c->heads[0].layers[1].out + c->heads[1].layers[1].out, K = S0.in;
        launch_gemm(st, c->dy_all, nt, c->weff, nt, nullptr, dfeat, K, rows, K, nt, 1, 0, 0);
        // their weight gradients (side stream) are enqueued behind the fork that follows the last GRU layer's BPTT: one
        // cross-stream event (a ~7 us bubble on the main stream) fewer
    } else if (heads_general(c)) {
        for (int hd = 0; hd < 2; ++hd) {
            Head& Hd = c->heads[hd];
            for (int j = (int)Hd.layers.size() - 1; j >= 0; --j) {
                DenseL& D = Hd.layers[j];
                float* din = j == 0 ? dfeat : Hd.layers[j - 1].dy;
                const int accumulate = (j == 0 && hd == 1) ? 1 : 0;
                if (D.ks > 1) {
                    launch_gemm(st, D.dy, D.out, c->params + D.w_off, D.out, nullptr, c->head_tmp, D.in, rows, D.in, D.out, 1, 0, 0);
                    launch_time_fold(st, c->head_tmp, din, c->B, c->S, D.in_base, D.ks, accumulate);
                } else {
                    launch_gemm(st, D.dy, D.out, c->params + D.w_off, D.out, nullptr, din, D.in, rows, D.in, D.out, 1, 0, accumulate);
                }
                if (j > 0) {
                    const DenseL& P = Hd.layers[j - 1];
                    const int64_t n = (int64_t)rows * P.out;
                    // the previous layer's dropout (the mask recomputed from the counters of the forward pass), then its activation
                    if (P.rate > 0.f && c->last_training) launch_dropout(st, din, din, n, P.rate, c->dropout_seed, P.drop_id, c->dropout_cur);
                    if (Hd.hidden_act) launch_act_bwd(st, P.y, din, n, Hd.hidden_act);
                }
            }
        }
        fork_side(c);
        for (int hd = 0; hd < 2; ++hd) {
            Head& Hd = c->heads[hd];
            for (int j = (int)Hd.layers.size() - 1; j >= 0; --j) {
                DenseL& D = Hd.layers[j];
                const float* ain = D.ks > 1 ? D.xe
                                 : (j == 0 ? Glast.out : (Hd.layers[j - 1].rate > 0.f && c->last_training ? Hd.layers[j - 1].yd : Hd.layers[j - 1].y));
                wgrad_dense(c, c->side, c->tn_slab_side, ain, D.in, D.dy, D.out, rows, D.in, D.out, D.w_off, D.b_off, 0, 0);
            }
        }
    } else {
    // the gradient w.r.t. the shared features is the sum over the two heads' first layers: one product over the
    // concatenated K axis when their shapes agree (out % 32 == 0), otherwise two launches with accumulation
    const bool merged0 = S0.in == D0.in && S0.out == D0.out && (S0.out & 31) == 0;
    for (int hd = 0; hd < 2; ++hd) {
        Head& Hd = c->heads[hd];
        for (int j = (int)Hd.layers.size() - 1; j >= (merged0 ? 1 : 0); --j) {
            DenseL& D = Hd.layers[j];
            float* din = j == 0 ? dfeat : Hd.layers[j - 1].dy;
            const int accumulate = (j == 0 && hd == 1) ? 1 : 0;
            launch_gemm(st, D.dy, D.out, c->params + D.w_off, D.out, nullptr, din, D.in, rows, D.in, D.out, 1, 0, accumulate);
            // through the hidden layer's dense_activation: the gradient w.r.t. its pre-activation, from its stored output
            if (j > 0 && Hd.hidden_act) launch_act_bwd(st, Hd.layers[j - 1].y, din, (int64_t)rows * D.in, Hd.hidden_act);
        }
    }
    if (merged0 && heads_sb(c) && gemm_sb_usable(S0.dy, S0.out, S0.in, S0.out) && gemm_sb_usable(D0.dy, S0.out, S0.in, S0.out)) {
        launch_gemm_sb(st, c->kc, true, GemmEpi(), S0.dy, D0.dy, S0.out, c->h0sp_bwd[0], c->h0sp_bwd[1], nullptr, nullptr, dfeat, nullptr, S0.in, rows, S0.in,
                       S0.out, 0, 2);
    } else if (merged0)
        launch_gemm_dual_k(st, S0.dy, D0.dy, S0.out, c->params + S0.w_off, c->params + D0.w_off, S0.out, nullptr, dfeat, S0.in, rows,
                           S0.in, S0.out, 1, 0, 0);
    fork_side(c);
    for (int hd = 0; hd < 2; ++hd) {
        Head& Hd = c->heads[hd];
        for (int j = (int)Hd.layers.size() - 1; j >= 0; --j) {
            DenseL& D = Hd.layers[j];
            const float* ain = j == 0 ? Glast.out : Hd.layers[j - 1].y;
            wgrad_dense(c, c->side, c->tn_slab_side, ain, D.in, D.dy, D.out, rows, D.in, D.out, D.w_off, D.b_off, 0, 0);
        }
    }
    }
    return SELD_OK;
}

// GRU layers, last to first.  dfeat = gradient w.r.t. the last layer's output; *din = gradient w.r.t. the first layer's input
static int backward_gru(seld_ctx* c, const float* dfeat, const float** din) {
    hipStream_t st = c->stream;
    const int B = c->B, S = c->S, rows = B * S;
    const float* dout = dfeat;
    for (int i = (int)c->gru.size() - 1; i >= 0; --i) {
        GruL& G = c->gru[i];
        const bool conv_drop = c->last_training && c->arch.conv_dropout > 0.f, gru_drop = c->last_training && c->arch.gru_dropout > 0.f;
        const float* lin = i == 0 ? (c->arch.first_kind == SELD_FIRST_XCEPTION ? c->xc_feat : (c->arch.first_kind == SELD_FIRST_RESNET50 ? c->rn.back().out : (conv_drop ? c->conv.back().pd : c->conv.back().p))) : c->gru[i - 1].out;
        {
            PROF(c, "gru_bwd");
            if (gru_drop) {
                if (launch_gru_bwd(st, GRU_BWD_MUL, dout, nullptr, G.h[0], G.h[1], G.sv[0], G.sv[1], c->params + G.u_off[0], c->params + G.u_off[1],
                                   c->dgx[i][0], c->dgx[i][1], c->dgh[i][0], c->dgh[i][1], B, S, G.rmask[0], G.rmask[1], G.hm[0], G.hm[1]))
                    return fail(c, SELD_ERR_UNSUPPORTED, "gru_bwd (dropout)");
            } else
            launch_gru_bwd(st, GRU_BWD_MUL, dout, nullptr, G.h[0], G.h[1], G.sv[0], G.sv[1], c->params + G.u_off[0], c->params + G.u_off[1],
                           c->dgx[i][0], c->dgx[i][1], c->dgh[i][0], c->dgh[i][1], B, S);
        }
        // the input gradient the next BPTT (or the conv backward) waits for: main stream, enqueued AFTER the side stream is released for this layer's weight
        // gradients (ahead of the release: same box 2.651 / 2.650 ms per step against 2.639 / 2.635 — what the product gains the weight gradients lose under the next BPTT)
        auto din_gemm = [&]() {
        {
            PROF2(c, "gru_bwd_gemms");   // main stream: the input gradient the next BPTT waits for
            // din = dgx_f K_f^T + dgx_b K_b^T: one product over the concatenated K axis (no read-modify-write of din)
            if (gru_drop) {      // din = (dgx_f K_f^T) * imask_f + (dgx_b K_b^T) * imask_b: each direction's input rows had their own mask
                for (int d = 0; d < 2; ++d) {
                    float* t_ = d == 0 ? G.din : G.dtmp;
                    if (gru_sb(c, G))
                        launch_gemm_sb(st, c->kc, true, GemmEpi(), c->dgx[i][d], nullptr, 384, c->ksp_bwd[i][d], nullptr, nullptr, nullptr, t_, nullptr, G.in_feat, rows, G.in_feat, 384, 0, 0);
                    else
                        launch_gemm(st, c->dgx[i][d], 384, c->params + G.k_off[d], 384, nullptr, t_, G.in_feat, rows, G.in_feat, 384, 1, 0, 0);
                    launch_mask_rows(st, t_, G.imask[d], G.din, rows, S, G.in_feat, d);
                }
            } else if (gru_sb(c, G)) {
                launch_gemm_sb(st, c->kc, true, GemmEpi(), c->dgx[i][0], c->dgx[i][1], 384, c->ksp_bwd[i][0], c->ksp_bwd[i][1], nullptr, nullptr, G.din, nullptr,
                               G.in_feat, rows, G.in_feat, 384, 0, 2);
            } else
                launch_gemm_dual_k(st, c->dgx[i][0], c->dgx[i][1], 384, c->params + G.k_off[0], c->params + G.k_off[1], 384, nullptr,
                                   G.din, G.in_feat, rows, G.in_feat, 384, 1, 0, 0);
        }
        };
        // weight gradients of this layer: side stream (they overlap with the next layer's BPTT, which uses 2B of the 256 CUs)
        fork_side(c);
        if (i == (int)c->gru.size() - 1 && heads_lin(c)) heads_lin_side(c, rows);
        TnJobs tj = {};
        for (int d = 0; d < 2; ++d) {
            // kernel + input bias (bias row 0); recurrent kernel: H_prev^T dgh (forward direction saw h[t-1], backward direction
            // h[t+1]) + bias row 1
            tj.A[2 * d] = gru_drop ? G.xm[d] : lin; tj.lda[2 * d] = G.in_feat; tj.B[2 * d] = c->dgx[i][d]; tj.shift[2 * d] = 0;
            tj.out_w[2 * d] = c->grads + G.k_off[d]; tj.out_b[2 * d] = c->grads + G.b_off[d];
            tj.A[2 * d + 1] = gru_drop ? G.hm[d] : G.h[d]; tj.lda[2 * d + 1] = 128; tj.B[2 * d + 1] = c->dgh[i][d]; tj.shift[2 * d + 1] = d == 0 ? -1 : 1;
            tj.out_w[2 * d + 1] = c->grads + G.u_off[d]; tj.out_b[2 * d + 1] = c->grads + G.b_off[d] + 384;
        }
        int ns4 = 0;
        if (c->gru_wgrad_batch && c->gemm_split_bf16 && G.in_feat == 128 && launch_gemm_tn_sb_batch(c->side, c->kc, tj, 4, 384, c->tn_slab_side, &ns4, rows, 384, S, 1) == 0) {
            // the layer's four products in one launch, their slabs combined by one more
            launch_reduce_slabs2_batch(c->side, c->tn_slab_side, ns4, (int64_t)128 * 384 + 384, tj, 4, (int64_t)128 * 384, 384);
        } else
            for (int j = 0; j < 4; ++j)
                wgrad_dense(c, c->side, c->tn_slab_side, tj.A[j], tj.lda[j], tj.B[j], 384, rows, j & 1 ? 128 : G.in_feat, 384,
                            tj.out_w[j] - c->grads, tj.out_b[j] - c->grads, j & 1 ? S : 0, tj.shift[j]);
        hipEventRecord(c->ev_bucket[(int)c->gru.size() - 1 - i], c->side);   // this layer's (and, for the last layer, the heads') gradients are final
        din_gemm();
        dout = G.din;
    }
    *din = dout;
    return SELD_OK;
}

// resnet50_block backward, blocks last to first; g = gradient w.r.t. the block's output, starting from dout.  *dp = gradient w.r.t. the
// entry block's output
static int backward_resnet(seld_ctx* c, const float* dout, const float** dp) {
    hipStream_t st = c->stream;
    const int B = c->B, S = c->S;
    PROF(c, "rn_stages_bwd");
    const bool sb = c->rn_split_bf16 != 0;
    // The kernel gradients (a third of the block's products) go to the side stream: one product of these shapes leaves the card
    // part-filled (e.g. 300 row tiles on 256 CUs), and an independent stream fills what the input-gradient chain leaves idle.
    // A dz buffer is handed over by ev_rn_ready and comes back by ev_rn_free[slot] before its next writer starts.
    const bool aside = c->rn_wgrad_side != 0;
    hipStream_t ws = aside ? c->side : st;
    bool busy[5] = {};
    int zi = 1, bbi = 4;        // last slot taken of rn_bz (0-1) / rn_bb (2-4)
    auto take = [&](int first, int n, int& cur) {
        cur = first + (cur - first + 1) % n;
        if (busy[cur]) { hipStreamWaitEvent(st, c->ev_rn_free[cur], 0); busy[cur] = false; }
        return cur < 2 ? c->rn_bz[cur] : c->rn_bb[cur - 2];
    };
    auto fork = [&](int) { if (aside) { hipEventRecord(c->ev_rn_ready, st); hipStreamWaitEvent(c->side, c->ev_rn_ready, 0); } };
    auto done = [&](int slot) { if (aside) { hipEventRecord(c->ev_rn_free[slot], c->side); busy[slot] = true; } };
    auto wgrad = [&](int slot, const float* A, int lda, const float* dz, int M_, int K1, int N, int64_t w_off) {
        fork(slot);
        launch_rn_product_wgrad(ws, c->kc, A, lda, dz, c->tn_slab, tn_slab_capacity(), c->grads + w_off, M_, K1, N,
                                c->rn_split_bf16);
        done(slot);
    };
    const float* g = dout;
    int flip = 0;
    for (int bi = (int)c->rn.size() - 1; bi >= 0; --bi) {
        if (c->sync_failed) break;     // a failed SyncBN collective: enqueue nothing further (the error is reported below)
        RnBlock& R = c->rn[bi];
        const int64_t M = (int64_t)B * S * R.Wout;
        const int w = R.w;
        const float* X = bi == 0 ? c->conv[0].p : c->rn[bi - 1].out;
        float* dX = bi == 0 ? c->conv[0].dp : c->rn_gx[flip];
        const int ldx = R.Cin * R.stride_f;
        // main branch: BN2 (behind the block's ReLU: mask = out), 1x1 expand
        float* dz2 = take(0, 2, zi);
        { PROF3(c, "rn_bn_bwd"); rn_bn_bwd(c, st, R.c[2], g, R.gate, dz2, M); }
        wgrad(zi, R.y1, w, dz2, (int)M, w, 4 * w, R.c[2].w_off);
        { PROF3(c, "rn_products_dgrad"); launch_rn_product_dgrad(st, c->kc, dz2, c->params + R.c[2].w_off, sb ? R.c[2].wsp_t : nullptr, c->rn_ba, w, (int)M, w, 4 * w, 0); }
        // BN1 (mask = y1), 3x3: stage 1 on the conv blocks' kernels, the other widths through im2col / col2im
        float* dz1 = take(2, 3, bbi);
        { PROF3(c, "rn_bn_bwd"); rn_bn_bwd(c, st, R.c[1], c->rn_ba, nullptr, dz1, M); }
        if (sb && rn_c1_direct(R)) {
            fork(bbi);
            int ns = 0;
            launch_conv64_wgrad_sb(ws, c->kc, R.y0, dz1, c->rn_w9_slab, &ns, B, S, rn_c1_width(R));
            if (R.c[1].w2) {
                launch_reduce_slabs(ws, c->rn_w9_slab, ns, 9 * 4096 + 64, R.c[1].dw2, 9 * 4096, 0);
                launch_rn_w32_extract(ws, R.c[1].dw2, c->grads + R.c[1].w_off);
            } else
                launch_reduce_slabs(ws, c->rn_w9_slab, ns, 9 * 4096 + 64, c->grads + R.c[1].w_off, 9 * 4096, 0);
            done(bbi);
            { PROF3(c, "rn_products_dgrad"); launch_conv64_dgrad_sb(st, c->kc, dz1, R.c[1].wsp9_flip, c->rn_ba, B, S, rn_c1_width(R)); }
        } else if (sb && rn_c1_implicit(c, R)) {
            fork(bbi);
            launch_rn_conv3_wgrad(ws, c->kc, R.y0, dz1, c->tn_slab, tn_slab_capacity(), c->grads + R.c[1].w_off, B, S,
                                  R.Wout, w, w);
            done(bbi);
            { PROF3(c, "rn_products_dgrad"); launch_rn_conv3_dgrad(st, c->kc, dz1, R.c[1].wsp_t, c->rn_ba, B, S, R.Wout, w, w); }
        } else {
            if (!R.c[1].col) return fail(c, SELD_ERR_INVALID, "resnet50_block: the options changed between forward and backward");
            if (!c->rn_bcol && dalloc(c, &c->rn_bcol, c->rn_col_elems)) return fail(c, SELD_ERR_NOMEM, "col2im tensor");
            wgrad(bbi, R.c[1].col, 9 * w, dz1, (int)M, 9 * w, w, R.c[1].w_off);
            { PROF3(c, "rn_products_dgrad"); launch_rn_product_dgrad(st, c->kc, dz1, c->params + R.c[1].w_off, sb ? R.c[1].wsp_t : nullptr, c->rn_bcol, 9 * w, (int)M, 9 * w, w, 0); }
            launch_col2im3x3(st, c->rn_bcol, c->rn_ba, B, S, R.Wout, w);
        }
        // BN0 (mask = y0), 1x1 reduce; its input gradient lands on the strided rows of dX
        float* dz0 = take(2, 3, bbi);
        { PROF3(c, "rn_bn_bwd"); rn_bn_bwd(c, st, R.c[0], c->rn_ba, nullptr, dz0, M); }
        wgrad(bbi, X, ldx, dz0, (int)M, R.Cin, w, R.c[0].w_off);
        if (R.stride_f > 1) hipMemsetAsync(dX, 0, (size_t)B * S * R.Win * R.Cin * sizeof(float), st);
        // identity block: the shortcut's gated gradient g [gate] is added in this product's epilogue (split-bf16 kernels; 1 = the shape took the
        // fp32 GEMM and the separate pass below still runs)
        const bool epi_add = !R.proj && c->rn_epi_add && R.stride_f == 1;
        int added = 1;
        { PROF3(c, "rn_products_dgrad"); added = launch_rn_product_dgrad(st, c->kc, dz0, c->params + R.c[0].w_off, sb ? R.c[0].wsp_t : nullptr, dX, ldx, (int)M, R.Cin, w, 0,
                                                                         epi_add ? g : nullptr, epi_add ? R.gate : nullptr); }
        if (added < 0) return fail(c, SELD_ERR_INVALID, "resnet50_block: reduce convolution's input-gradient product");
        // shortcut
        if (R.proj) {
            float* dzs = take(0, 2, zi);
            { PROF3(c, "rn_bn_bwd"); rn_bn_bwd(c, st, R.sc, g, R.gate, dzs, M); }
            wgrad(zi, X, ldx, dzs, (int)M, R.Cin, 4 * w, R.sc.w_off);
            { PROF3(c, "rn_products_dgrad"); launch_rn_product_dgrad(st, c->kc, dzs, c->params + R.sc.w_off, sb ? R.sc.wsp_t : nullptr, dX, ldx, (int)M, R.Cin, 4 * w, 1); }
        } else if (!epi_add || added == 1) {
            { PROF3(c, "rn_bn_bwd"); launch_rn_add_gated(st, dX, g, R.gate, M * 4 * w); }
        }
        g = dX;
        flip ^= 1;
    }
    if (c->sync_failed) { c->sync_failed = false; return fail(c, SELD_ERR_HIP, "sync_bn all-reduce callback failed"); }
    *dp = c->conv[0].dp;
    return SELD_OK;
}

// xception_block backward: exit pool (from dout), then the modules last to first.  gX = gradient w.r.t. the module's output
// (= the next module's input); within a module gY walks back through the three units and the residual adds gX to it.
// *dp = gradient w.r.t. the entry block's output
static int backward_xception(seld_ctx* c, const float* dout, const float** dp) {
    hipStream_t st = c->stream;
    const int B = c->B, S = c->S;
    const int64_t npix = (int64_t)B * S * 16;
    // three [B,S,16,64] gradient buffers: X = gradient w.r.t. the current module's output (kept until its residual add),
    // F1 = gradient w.r.t. a unit's depthwise output, F2 = gradient w.r.t. a unit's input (= the previous unit's output)
    float *X = c->xc_g[0], *F1 = c->xc_g[1], *F2 = c->xc_g[2];
    {
        PROF2(c, "xc_exit_pool_bwd");
        const float* id = c->xc_ident;       // mean 0 | invstd 1 | scale 1 | shift 0 | c1 0 | c2 0
        launch_bn_pool_bwd_dz(st, c->xc_x.back(), dout, id, id + 64, id + 128, id + 192, id + 256, X, B, S, 16, 64, 1, 8);
    }
    // The two kernel gradients of a unit (pointwise: dwo^T dz, depthwise: from the unit's input and F1) are off the input-gradient
    // chain: they run on the side stream; dz and F1 alternate between two buffers each, handed over by ev_rn_ready and taken back
    // by ev_rn_free[slot] (slots 0-1 dz, 2-3 F1) before the buffer's next writer starts.
    const bool aside = c->xc_wgrad_side != 0;
    hipStream_t ws = aside ? c->side : st;
    float* dzb[2] = {c->dzbuf, c->xc_dz2};
    float* f1b[2] = {F1, c->xc_g[3]};
    bool busy[4] = {};
    int di = 1, fi = 1;
    auto take = [&](int first, int& cur) {
        cur ^= 1;
        if (busy[first + cur]) { hipStreamWaitEvent(st, c->ev_rn_free[first + cur], 0); busy[first + cur] = false; }
        return first + cur;
    };
    auto fork = [&]() { if (aside) { hipEventRecord(c->ev_rn_ready, st); hipStreamWaitEvent(c->side, c->ev_rn_ready, 0); } };
    auto done = [&](int slot) { if (aside) { hipEventRecord(c->ev_rn_free[slot], c->side); busy[slot] = true; } };
    bool have_sums = false;      // the running unit's BatchNorm-backward partials are in xc_part_dw (n_dw_part rows)
    int n_dw_part = 0;
    struct { float* slab; int ns_pw, ns_dw; int64_t pw_off, dw_off; } pend[3];      // xc_nowait: a module's combines, launched behind its last unit
    int npend = 0;
    for (int b = (int)c->arch.xc_blocks - 1; b >= 0; --b) {
        const float* gY = X;
        for (int u = 2; u >= 0; --u) {
            XcUnit& U = c->xc[(size_t)b * 3 + u];
            const bool fold = c->xc_fused_fwd && u > 0;       // the forward applied the previous unit's BatchNormalization on load
            const float* uin = u == 0 ? c->xc_x[b] : (fold ? c->xc[(size_t)b * 3 + u - 1].z : c->xc[(size_t)b * 3 + u - 1].a);
            const float* aff = fold ? c->xc[(size_t)b * 3 + u - 1].scale : nullptr;
            int np = 0, ns = 0, ns_pw = 0;
            const bool fpw = c->xc_fused_pw_bwd != 0;
            int sd = -1;
            float* dz = nullptr;
            if (!fpw) { sd = take(0, di); dz = dzb[di]; }
            {
                PROF2(c, "xc_bn_bwd");
                // the sums [sum gY | sum gY xhat]: left by the depthwise input-gradient pass that produced gY (have_sums), else a pass over (z, gY)
                if (have_sums) launch_xc_fold_partials(st, c->xc_part_dw, n_dw_part, c->xc_part, &np);
                else launch_xc_bn_bwd_reduce(st, U.z, gY, U.mean, U.invstd, c->xc_part, &np, npix);
                have_sums = false;
                if (c->sync_fn) {
                    launch_bn_partials_to_sums(st, c->xc_part, np, c->sync_buf, (double)npix);
                    launch_bn_bwd_local(st, c->sync_buf, c->grads + U.g_off, c->grads + U.be_off);
                    if (c->sync_fn(c->sync_user, c->sync_buf, 129, SELD_DTYPE_F64, st)) return fail(c, SELD_ERR_HIP, "sync_bn all-reduce callback failed");
                    launch_bn_bwd_c1c2(st, c->sync_buf, 0.0 /* the all-reduced count */, U.c1c2);
                } else
                    launch_bn_bwd_finalize(st, c->xc_part, np, (double)npix, c->grads + U.g_off, c->grads + U.be_off, U.c1c2, 64);
                if (!fpw) launch_xc_bn_bwd_dz(st, U.z, gY, U.mean, U.invstd, U.scale, U.c1c2, dz, npix);
            }
            // xc_nowait: the default path's side-stream work reads slab buffers only, and every unit has its own: no slot to take back
            const bool nowait = fpw && c->xc_fused_dw_bwd && c->xc_nowait && c->xc_unit_slab;
            float* uslab = nowait ? c->xc_unit_slab + ((size_t)b * 3 + u) * c->xc_unit_slab_per : nullptr;
            int sf = -1;
            if (nowait) fi ^= 1; else sf = take(2, fi);
            float* F1c = f1b[fi];
            if (nowait) {
                PROF2(c, "xc_pointwise_bwd");
                launch_xc_pw_bwd(st, U.z, gY, U.dwo, c->params + U.pw_off, U.mean, U.invstd, U.scale, U.c1c2, F1c, uslab, &ns_pw, npix);
            } else if (fpw) {
                PROF2(c, "xc_pointwise_bwd");
                // dz formed on load; F1 = dz W^T and the slabs of dW = dwo^T dz from one pass (xc_pw_bwd); the combine goes to the side stream
                if (busy[0]) { hipStreamWaitEvent(st, c->ev_rn_free[0], 0); busy[0] = false; }      // slot 0 = the slab buffer here
                launch_xc_pw_bwd(st, U.z, gY, U.dwo, c->params + U.pw_off, U.mean, U.invstd, U.scale, U.c1c2, F1c, c->tn_slab, &ns, npix);
                fork();
                launch_reduce_slabs(ws, c->tn_slab, ns, 4096, c->grads + U.pw_off, 4096, 0);
                done(0);
            } else {
                PROF2(c, "xc_pointwise_bwd");
                // dW = dwo^T dz (TN product over the pixels, many short splits: the slab is only 64 x 64), d(dwo) = dz W^T
                fork();
                launch_gemm_tn(ws, U.dwo, 64, dz, 64, c->tn_slab, &ns, (int)npix, 64, 64, 0, 0, 0, 512);
                launch_reduce_slabs2(ws, c->tn_slab, ns, 64 * 64 + 64, c->grads + U.pw_off, 64 * 64, nullptr, 0);
                done(sd);
                launch_gemm(st, dz, 64, c->params + U.pw_off, 64, nullptr, F1c, 64, (int)npix, 64, 64, 1, 0, 0);
            }
            PROF2(c, "xc_depthwise_bwd");
            // gradient w.r.t. the unit's input, through its ReLU; the module's first unit adds the residual branch's X
            float* gin = (u == 0 && b == 0) ? c->conv[0].dp : F2;
            if (c->xc_fused_dw_bwd) {
                // ... and the kernel-gradient slabs from the same pass (slab buffer fi: slot `sf` was taken above, i.e. its last combine is done)
                float* sl = nowait ? uslab + c->xc_unit_slab_pw : c->xc_slab + (size_t)fi * c->xc_slab_per;
                // a folded unit's input is the previous unit's pre-BN tensor and gin that BatchNormalization's output gradient: its backward sums ride along
                const bool sums = fold && c->xc_fused_bn_sums;
                const XcUnit* Pv = sums ? &c->xc[(size_t)b * 3 + u - 1] : nullptr;
                if (launch_dw3x3_bwd_fused(st, c->kc, F1c, c->params + U.dw_off, uin, u == 0 ? X : nullptr, gin, sl, &ns, B, S, 16, aff,
                                           sums ? Pv->mean : nullptr, sums ? Pv->invstd : nullptr, sums ? c->xc_part_dw : nullptr))
                    return fail(c, SELD_ERR_UNSUPPORTED, "dw3x3_bwd_fused");
                if (sums) { have_sums = true; n_dw_part = ns; }
                if (nowait) {
                    // ONE hand-over per module (an event record costs the main stream ~5 us): the three units' combines go to the side stream behind the
                    // module's last unit, each on buffers of its own
                    pend[npend++] = {uslab, ns_pw, ns, U.pw_off, U.dw_off};
                    if (u == 0) {
                        fork();
                        for (int q = 0; q < npend; ++q) {
                            float* tmp_ = pend[q].slab + c->xc_unit_slab_pw + c->xc_unit_slab_dw;
                            launch_reduce_slabs_2stage(ws, pend[q].slab, pend[q].ns_pw, 4096, c->grads + pend[q].pw_off, 4096, tmp_ + (size_t)reduce_slabs_groups(xc_dw_fused_slabs(c->Bmax, c->S)) * 576);
                            launch_reduce_slabs_2stage(ws, pend[q].slab + c->xc_unit_slab_pw, pend[q].ns_dw, 576, c->grads + pend[q].dw_off, 576, tmp_);
                        }
                        npend = 0;
                    }
                } else {
                    fork();
                    launch_reduce_slabs_2stage(ws, sl, ns, 576, c->grads + U.dw_off, 576, c->xc_slab_tmp);      // side stream: its launches are ordered, one tmp
                    done(sf);
                }
            } else {
                fork();
                launch_dw3x3_bwd_w(ws, uin, F1c, c->xc_slab, &ns, B, S, 16, aff);
                launch_reduce_slabs(ws, c->xc_slab, ns, 576, c->grads + U.dw_off, 576, 0);
                done(sf);
                launch_dw3x3_bwd_data(st, c->kc, F1c, c->params + U.dw_off, uin, u == 0 ? X : nullptr, gin, B, S, 16, aff);
            }
            gY = gin;
        }
        if (b > 0) { float* t_ = X; X = F2; F2 = t_; }      // the module's input gradient is the next module's output gradient
    }
    // the first block's backward (main stream) writes dzbuf: not before the side stream's last reader of it is done
    for (int k = 0; k < 4; ++k)
        if (busy[k]) hipStreamWaitEvent(st, c->ev_rn_free[k], 0);
    *dp = c->conv[0].dp;
    return SELD_OK;
}

// conv blocks, last to first.  dp = gradient w.r.t. the last block's (pooled, dropped-out) output; x = the forward pass's input
static int backward_conv_blocks(seld_ctx* c, const float* x, const float* dp) {
    hipStream_t st = c->stream;
    const int B = c->B;
    const bool conv_drop = c->last_training && c->arch.conv_dropout > 0.f;
    bool dz_busy[2] = {false, false};      // conv_wgrad_side: a side-stream kernel gradient reads dzbuf / dzbuf_alt (ev_rn_free[0 / 1] marks its end)
    for (int i = (int)c->conv.size() - 1; i >= 0; --i) {
        ConvL& L = c->conv[i];
        int np = 0;
        char tn[32];
        snprintf(tn, sizeof tn, "pool%d_bwd_reduce", i + 1);
        if (conv_drop) {      // through this block's Dropout: the forward's draws again (in place: dp is a buffer of this context)
            float* g_ = const_cast<float*>(dp);
            launch_dropout(st, g_, g_, (int64_t)B * (L.H / L.pt) * (L.W / L.pf) * 64, c->arch.conv_dropout, c->dropout_seed, 64u + (unsigned)i, c->dropout_cur);
        }
        {
            PROF2(c, tn);
            const bool gz = i == 0 && c->gram_active;      // no z: the windows' extreme values stand in
            if (launch_bn_pool_bwd_reduce(st, gz ? L.zext : L.z, L.p, dp, L.mean, L.invstd, L.scale, L.shift, c->bn_partial, &np, B,
                                          L.H, L.W, 64, L.pt, L.pf, gz ? 1 : 0))
                return fail(c, SELD_ERR_UNSUPPORTED, "bn_pool_bwd_reduce");
        }
        if (c->sync_fn) {
            launch_bn_partials_to_sums(st, c->bn_partial, np, c->sync_buf, (double)B * L.H * L.W);
            launch_bn_bwd_local(st, c->sync_buf, c->grads + L.g_off, c->grads + L.be_off);
            if (c->sync_fn(c->sync_user, c->sync_buf, 129, SELD_DTYPE_F64, st)) return fail(c, SELD_ERR_HIP, "sync_bn all-reduce callback failed");
            launch_bn_bwd_c1c2(st, c->sync_buf, 0.0 /* the all-reduced count */, L.c1c2);
        } else
            launch_bn_bwd_finalize(st, c->bn_partial, np, (double)B * L.H * L.W, c->grads + L.g_off, c->grads + L.be_off, L.c1c2, 64);
        int ns = 0;
        // conv_wgrad_side (round 5; same box 2.551 -> 2.523 ms): blocks 2 / 3 put their kernel gradient on the side stream (idle in this part of the step); their dz then
        // alternates between two buffers — the next block's dz is written while the side stream still reads this one's — and the slabs are the side stream's own
        const bool wside = c->conv_wgrad_side && c->prof < 2 && i >= 1 && c->dzbuf_alt && c->wgrad_slab_side;      // (a level-2 profile pass times every kernel alone)
        const int dzpar = (wside && (i & 1)) ? 1 : 0;
        float* dzb = dzpar ? c->dzbuf_alt : c->dzbuf;
        const bool fused_first = (i == 0) && L.pf == 4 && (L.pt == 5 || L.pt == 4 || L.pt == 2 || L.pt == 1);
        if (!fused_first) {
            snprintf(tn, sizeof tn, "pool%d_bwd_dz", i + 1);
            PROF2(c, tn);
            // a kernel gradient on the side stream may still read this buffer (two blocks back, or the third block's when the first block's dz goes here)
            if (dz_busy[dzpar]) { hipStreamWaitEvent(st, c->ev_rn_free[dzpar], 0); dz_busy[dzpar] = false; }
            launch_bn_pool_bwd_dz(st, L.z, dp, L.mean, L.invstd, L.scale, L.shift, L.c1c2, dzb, B, L.H, L.W, 64, L.pt, L.pf);
        }
        if (i == 0 && c->gram_active) {
            PROF(c, "conv1_wgrad");
            // dW = ka (G W + g b) + g kb + M  (conv_gram.hip): M from x, the pooled gradient and the recorded argmax
            const int kp = conv_gram_dim(L.Cin);
            if (launch_conv_first_msparse(st, x, L.p, dp, L.amax, L.scale, c->wgrad_slab, &ns, B, L.H, L.Cin))
                return fail(c, SELD_ERR_UNSUPPORTED, "conv_first_msparse");
            launch_reduce_slabs(st, c->wgrad_slab, ns, (int64_t)kp * 64, c->mmat, (int64_t)kp * 64, 0);
            hipStreamWaitEvent(st, c->ev_gram, 0);
            launch_conv_first_assemble(st, c->gram, c->mmat, c->params + L.w_off, c->params + L.b_off, L.mean, c->grads + L.w_off,
                                       c->grads + L.b_off, L.Cin);
        } else if (i == 0) {
            {
                PROF(c, "conv1_wgrad");
                // fused: dz = BN/ReLU/pool backward formed inside the wgrad kernel (L.mean.. are contiguous: 6 x 64)
                const int rc = fused_first
                    ? launch_conv_first_wgrad_fused(st, x, L.z, L.p, dp, L.amax, L.mean, c->wgrad_slab, &ns, B, L.H, L.Cin, L.pt, L.pf)
                    : launch_conv_first_wgrad(st, x, c->dzbuf, c->wgrad_slab, &ns, B, L.H, L.Cin);
                if (rc) return fail(c, SELD_ERR_UNSUPPORTED, "conv_first_wgrad");
            }
            // slab rows 0..9*Cin-1 = kernel [9*Cin][64], row 9*Cin = bias: contiguous with the flat layout
            launch_reduce_slabs(st, c->wgrad_slab, ns, conv_first_wgrad_slab_stride(L.Cin), c->grads + L.w_off,
                                (int64_t)(9 * L.Cin + 1) * 64, 0);
        } else {
            const float* lin = conv_drop ? c->conv[i - 1].pd : c->conv[i - 1].p;
            snprintf(tn, sizeof tn, "conv%d_wgrad", i + 1);
            {
                PROF2(c, tn);
                hipStream_t wst = wside ? c->side : st;
                float* wsl = wside ? c->wgrad_slab_side : c->wgrad_slab;
                if (wside) { hipEventRecord(c->ev_fork, st); hipStreamWaitEvent(c->side, c->ev_fork, 0); }      // dz (and the block's input) are final on the main stream
                if (c->conv64_split_bf16 && conv64_wgrad_sb_usable(L.W)) {
                    if (launch_conv64_wgrad_sb(wst, c->kc, lin, dzb, wsl, &ns, B, L.H, L.W))
                        return fail(c, SELD_ERR_UNSUPPORTED, "conv64_wgrad_sb");
                } else if (launch_conv64_wgrad(wst, lin, dzb, wsl, &ns, B, L.H, L.W))
                    return fail(c, SELD_ERR_UNSUPPORTED, "conv64_wgrad");
                launch_reduce_slabs(wst, wsl, ns, 9 * 4096 + 64, c->grads + L.w_off, 9 * 4096 + 64, 0);
                if (wside) { hipEventRecord(c->ev_rn_free[dzpar], c->side); dz_busy[dzpar] = true; }      // this dz buffer's reader on the side stream
            }
            snprintf(tn, sizeof tn, "conv%d_dgrad", i + 1);
            {
                PROF2(c, tn);
                if (c->conv64_split_bf16) {   // flipped + split planes were made by the forward's weight pre-pass
                    launch_conv64_dgrad_sb(st, c->kc, dzb, c->wsp_bwd[i], c->conv[i - 1].dp, B, L.H, L.W);
                } else {
                    launch_flip_weights(st, c->params + L.w_off, c->wflip);
                    launch_conv64_fwd(st, dzb, c->wflip, nullptr, c->conv[i - 1].dp, nullptr, nullptr, B, L.H, L.W);
                }
            }
            dp = c->conv[i - 1].dp;
        }
    }
    return SELD_OK;
}

int backward_impl(seld_ctx* c, const float* x) {
    const float *dout = nullptr, *dp = nullptr;      // gradient w.r.t. the first GRU layer's input / the conv blocks' output
    int rc = apply_overrides(c);
    if (!rc) rc = backward_heads(c);
    if (!rc) rc = backward_gru(c, c->feat_grad, &dout);
    dp = dout;
    if (!rc && c->arch.first_kind == SELD_FIRST_RESNET50) rc = backward_resnet(c, dout, &dp);
    if (!rc && c->arch.first_kind == SELD_FIRST_XCEPTION) rc = backward_xception(c, dout, &dp);
    if (!rc) rc = backward_conv_blocks(c, x, dp);
    if (rc) return rc;
    // the deferred loss scalars (run_losses): the side stream is ordered behind the losses kernel by every fork above
    if (c->fin_sl)
        launch_losses_finalize(c->side, c->fin_doa_loss, c->den_dev, c->fin_sl, c->fin_dl, c->loss_scratch, c->B, c->S, c->arch.n_classes);
    c->fin_sl = nullptr;
    // join: the side stream's weight gradients must be complete before Adam / the DP all-reduce
    hipEventRecord(c->ev_join, c->side);
    hipStreamWaitEvent(c->stream, c->ev_join, 0);
    return check_launch(c, "backward");
}
