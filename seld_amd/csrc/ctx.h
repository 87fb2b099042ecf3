// ctx.h — the context (seld_ctx), its layer records and the small host helpers shared by the host files of libseld_hip.so:
// api.hip (the C ABI), forward.hip / backward.hip (the passes) and dp.hip (data parallelism).  Private to this directory.
#pragma once
#include "common.h"
#include "../../include/seld_hip.h"

#include <string>
#include <vector>

struct Var { std::string name; int64_t off; int rank; int64_t shape[4]; };

struct Timer { std::string name; std::vector<hipEvent_t> ev; int64_t launches = 0; double ms = 0.0; };

struct ConvL {
    int H, W, Cin, pt, pf;            // input geometry of this conv, pooling
    int64_t w_off, b_off, g_off, be_off;   // trainable offsets
    int64_t mm_off, mv_off;           // state offsets
    float *z = nullptr, *p = nullptr, *dp = nullptr;
    float* pd = nullptr;              // seld_arch.conv_dropout > 0: the block's output after Dropout (p stays the pooled tensor the backward reads)
    unsigned char* amax = nullptr;    // first block only: position of each pooling window's extreme [B,H/pt,W/pf,64]
    float* zext = nullptr;            // first block only: the windows' extreme z (kept next to p for the z-free backward)
    float *mean, *invstd, *scale, *shift, *c1c2;   // into small buffer
};

struct GruL {
    int in_feat;
    int64_t k_off[2], u_off[2], b_off[2];
    float *gx[2], *sv[2], *h[2], *out, *din;   // din: gradient w.r.t. this layer's input
    // seld_arch.gru_dropout > 0 (training): per direction the input mask [B][in_feat] and the state mask [B][128] (0 | 1/(1-rate)), the masked
    // input rows xm [rows][in_feat] (the kernel product's and the kernel gradient's operand), the masked state sequence hm [rows][128]
    // (h_prev of the backward pass and the recurrent-kernel gradient's operand); dtmp: the second direction's input gradient before its mask
    float *imask[2] = {}, *rmask[2] = {}, *xm[2] = {}, *hm[2] = {}, *dtmp = nullptr;
};

struct DenseL {
    int in, out; int64_t w_off, b_off; float* y; float* dy;      // in = the product's K (= ks * in_base)
    // simple_dense_block's hidden layers (modules.py:355-374): Conv1D kernel_size, Dropout rate; xe = the input rows laid side by side
    // [rows][ks * in_base] (ks > 1), yd = the layer's output after dropout (rate > 0), drop_id = the layer's dropout stream
    int ks = 1, in_base = 0; float rate = 0.f; float *xe = nullptr, *yd = nullptr; unsigned drop_id = 0;
};

// Conv2D(k in {1, 3}, strides (1, stride_f), use_bias=False) + BatchNormalization of resnet50_block (spec/RESNET50_BLOCK.md)
struct RnConv {
    int k = 1, Cin = 0, Cout = 0;
    int64_t w_off = 0, g_off = 0, be_off = 0, mm_off = 0, mv_off = 0;
    float *col = nullptr, *z = nullptr, *coef = nullptr;     // im2col of the input (k = 3), pre-BN output, [mean|invstd|scale|shift|c1|c2] x Cout
    unsigned short *wsp = nullptr, *wsp_t = nullptr;         // pre-split bf16 planes of the kernel / its transpose (shapes the split-bf16 GEMM takes)
    unsigned short *wsp9 = nullptr, *wsp9_flip = nullptr;    // 3x3, 64 -> 64 (stage 1): tap planes for the implicit-GEMM kernels of conv_sb.hip
    float *w2 = nullptr, *dw2 = nullptr;                     // 3x3, 32 -> 32 (stage 0): the kernel embedded as 64 -> 64 over pairs of bins, its gradient
};
struct RnBlock {
    int Cin, w, stride_f, Win, Wout;
    bool proj;
    RnConv c[3], sc;
    float *y0 = nullptr, *y1 = nullptr, *out = nullptr;      // ReLU(BN(c0)), ReLU(BN(c1)) [M, w]; block output [M, 4w]
    unsigned char* gate = nullptr;                          // [M, w]: bit j of byte q = (out[4 q + j] > 0), written by the forward's last pass
};

// one  ReLU -> SeparableConv2D(64, 3, use_bias=False) -> BatchNormalization  unit of xception_block's middle flow (spec/XCEPTION_BLOCK.md)
struct XcUnit {
    int64_t dw_off, pw_off, g_off, be_off;   // trainable offsets: depthwise_kernel [3,3,64,1], pointwise_kernel [1,1,64,64], gamma, beta
    int64_t mm_off, mv_off;                  // state offsets
    float *dwo = nullptr, *z = nullptr, *a = nullptr;   // depthwise output, pointwise output (pre-BN), unit output (units 0, 1)
    float *mean, *invstd, *scale, *shift, *c1c2;
};

struct Head {
    std::vector<DenseL> layers;   // dense chain, last = output layer with activation
    int act;
    int hidden_act = 0;           // simple_dense_block's dense_activation on the hidden layers (SELD_ACT_*; 0 = linear)
};

struct seld_ctx {
    seld_arch arch;
    int B, Bmax, T, S, device;
    hipStream_t stream = nullptr;
    std::vector<Var> tr, nt;
    int64_t nparam = 0, nstate = 0;
    float *params = nullptr, *grads = nullptr, *adam_m = nullptr, *adam_v = nullptr, *state = nullptr;
    int64_t adam_step = 0;
    std::vector<ConvL> conv;
    std::vector<GruL> gru;
    // test aid (seld_debug_set_routing / seld_debug_set_relu_gates): decisions the NEXT backward passes are told to take
    struct Override { int kind, block, which; int64_t n; int64_t* idx; unsigned char* val; };
    std::vector<Override> overrides;
    Head heads[2];
    // xception_block (arch.first_kind == SELD_FIRST_XCEPTION): conv[0] is the entry block, then 3 * xc_blocks units on [B,S,16,64]
    std::vector<XcUnit> xc;
    std::vector<float*> xc_x;                // [xc_blocks + 1] module inputs: xc_x[0] = conv[0].p, xc_x[b + 1] = xc_x[b] + y
    float *xc_small = nullptr, *xc_ident = nullptr, *xc_feat = nullptr, *xc_part = nullptr, *xc_slab = nullptr;
    float* xc_unit_slab = nullptr;    // xc_nowait: per unit [pointwise slabs | depthwise slabs | first-stage sums]
    size_t xc_unit_slab_per = 0, xc_unit_slab_pw = 0, xc_unit_slab_dw = 0;
    int xc_nowait = 1;
    float* xc_slab_tmp = nullptr;     // first-stage sums of the fused pass's slabs (launch_reduce_slabs_2stage)
    float* xc_part_dw = nullptr;      // BatchNorm-backward partials left by the fused depthwise input-gradient pass, one [128] per workgroup
    size_t xc_slab_per = 0;      // floats per depthwise-slab buffer (xc_slab holds two)
    float *xc_g[4] = {}, *xc_dz2 = nullptr;  // gradient ping-pong buffers [B,S,16,64] (X, F1, F2, second F1); second dz buffer
    int xc_fused_pw_bwd = 1;                 // a unit's BatchNorm' + pointwise input / kernel gradients in one kernel (xc_pw_bwd)
    int xc_wgrad_side = 1;                   // xception_block backward: kernel gradients on the side stream (as rn_wgrad_side)
    // resnet50_block (arch.first_kind == SELD_FIRST_RESNET50): conv[0] is the entry block, then the bottleneck blocks
    std::vector<RnBlock> rn;
    float *rn_part = nullptr, *rn_part_side = nullptr, *rn_gx[2] = {}, *rn_bz[2] = {}, *rn_ba = nullptr, *rn_bb[3] = {}, *rn_bcol = nullptr;
    size_t rn_part_floats = 0;     // floats each of rn_part / rn_part_side holds (seld_create: the most any statistics launch writes at Bmax, S)
    // resnet50_block backward: the kernel gradients run on the side stream beside the input-gradient chain; the dz buffers rotate
    // (ev_rn_free[slot]: the side stream's product that read the slot is done; slots 0-1 = rn_bz, 2-4 = rn_bb)
    hipEvent_t ev_rn_ready = nullptr, ev_rn_free[5] = {};
    float* rn_w9_slab = nullptr;           // slabs of the stage-1 3x3 kernel gradients (wgrad_slab belongs to the main stream's first block)
    int rn_wgrad_side = 1;
    size_t rn_col_elems = 0;
    int rn_implicit3x3 = 1;                // stages 2-3: the 3x3 products read im2col rows formed on load (0: materialised im2col / col2im)
    int rn_feat = 0;                         // features per label frame into the first GRU layer (2 x 32 rn_filters)
    float *feat_grad = nullptr;       // gradient w.r.t. the last pooled conv output ([B,S,128])
    float *dzbuf = nullptr, *small = nullptr, *stat_partial = nullptr, *bn_partial = nullptr;
    float *wgrad_slab = nullptr, *tn_slab = nullptr, *cs_slab = nullptr, *wflip = nullptr;
    float *wgrad_slab_side = nullptr, *dzbuf_alt = nullptr;      // conv_wgrad_side: the side stream's own slabs, the second dz buffer (allocated when the option is set)
    int conv_wgrad_side = 1;
    float *dgx[SELD_MAX_LAYERS][2] = {}, *dgh[SELD_MAX_LAYERS][2] = {};   // per GRU layer: the side stream reads them later
    float* tn_slab_side = nullptr;
    unsigned short* wsplit = nullptr;      // per 64->64 conv layer i: [2 i] forward, [2 i + 1] flipped; each [9][3][64][64] bf16 planes
    unsigned short *wsp_fwd[SELD_MAX_LAYERS] = {}, *wsp_bwd[SELD_MAX_LAYERS] = {};
    int conv1_gram = 1;                    // 1: first block's kernel gradient from the patch Gram matrix, no pre-BN tensor (conv_gram.hip)
    bool xc_fused_fwd = true;              // xception_block: depthwise + pointwise + BN statistics of a unit in one kernel
    int gram_parts = 2;                    // 2: the background Gram launch in two halves, one under each of the first two GRU layers' forward recurrences
    bool conv3_pre_fused = true;           // ... and the second block's (1,4) pooling pass: window extremes in its epilogue, BatchNorm + ReLU in the third block's loader
    bool conv2_pre_fused = true;           // the first block's BatchNorm + ReLU pass over its pooled tensor folded into the second block's region load
    bool gru_wgrad_batch = true;           // a GRU layer's four weight-gradient products in one launch (+ one combine)
    bool gram_active = false;              // the last training forward took that path
    float *gram_slab = nullptr, *gram = nullptr, *mmat = nullptr;
    hipEvent_t ev_gram = nullptr;
    int conv1_split_bf16 = 1;              // 1: the z-free first-block forward on bf16 MFMA with exactly split operands (conv_pool_sb.hip)
    int conv1_pool_fused = 1;              // 1: first block's (5,4) pool window reduction inside the conv epilogue (conv_pool.hip)
    int heads_fused = 1;                   // 1: heads of two LINEAR-then-activated layers run as one product with W1 W2 (see heads_lin)
    float *weff = nullptr, *dy_all = nullptr, *headF = nullptr;   // [K + 1][NT], [rows][NT], [K][NT] + [NT]
    int rn_split_bf16 = 1;                 // resnet50_block: products with N % 128 == 0 (stages 2-3, the expand / shortcut convolutions of
                                           // stages 0-1) on the split-bf16 kernels; 0: everything on the fp32 MFMA GEMM
    int gemm_split_bf16 = 1;               // 1: GRU input projections / heads' first Conv1D (and their input gradients) on the
                                           //    split-bf16 GEMM (gemm_sb.hip) where the shapes allow; 0: exact-fp32 MFMA GEMM
    unsigned short* gsplit = nullptr;      // pre-split weight operands of those products, refreshed by every forward
    unsigned short *ksp_fwd[SELD_MAX_LAYERS][2] = {}, *ksp_bwd[SELD_MAX_LAYERS][2] = {}, *h0sp_fwd[2] = {}, *h0sp_bwd[2] = {};
    int conv64_split_bf16 = 1;             // 1: conv2/conv3 forward + input gradient on bf16 MFMA with exact 3-way split operands
    hipStream_t side = nullptr;            // weight-gradient GEMMs run here, under the BPTT chain of the main stream
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_prep = nullptr;
    int prep_side = 0;      // option (off by default): the step's weight pre-pass on the side stream beside the first block's forward
    hipEvent_t ev_bucket[SELD_MAX_LAYERS] = {};   // side stream: GRU layer n_gru-1-k's (and, k = 0, the heads') gradients are final
    seld_allreduce_fn sync_fn = nullptr;          // synchronised BatchNorm (seld_set_sync_bn)
    void* sync_user = nullptr;
    int sync_world = 1;
    double* sync_buf = nullptr;                   // [128] (resnet50_block: [16][128]) sums handed to sync_fn
    bool sync_failed = false;                     // the all-reduce callback failed inside a helper: reported at the end of the pass
    // what the launchers choose their kernels by (common.h): seld_create (SELD_DTYPE_BF16 -> mfma_one) and seld_set_option write it, the passes hand it
    // to every launcher that reads a field — a context's arithmetic depends on nothing outside the context and the call
    KernelChoices kc;
    int xc_fused_bn_sums = 1;              // ... and, for a folded unit, the previous BatchNormalization's backward sums too (0: xc_reduce's pass over (z, gY))
    int xc_fused_dw_bwd = 1;               // xception_block: the depthwise kernel gradient's slabs come out of the input-gradient pass (round 5; 0: dw3x3_bwd_w on the side stream)
    int rn_epi_stats = 1;                  // resnet50_block: a convolution's BatchNorm statistics leave with its product's epilogue (round 5; 0: the separate pass over z)
    int rn_epi_add = 1;                    // ... and the identity shortcut's gated gradient is added in the reduce convolution's input-gradient epilogue
    // data parallelism inside the library (seld_dp_*): one RCCL communicator, a communication stream, two events
    void* dp_comm = nullptr;                      // ncclComm_t
    int dp_rank = 0, dp_world = 1;
    hipStream_t dp_stream = nullptr;
    hipEvent_t ev_dp_main = nullptr, ev_dp_done = nullptr;
    float *dsed_pre = nullptr, *ddoa_pre = nullptr, *sed_int = nullptr, *doa_int = nullptr;
    float *doa_v1 = nullptr;                   // models.seldnet_v1 (models.py:36-52): tanh(doa * [sed | sed | sed]), the prediction the losses see
    float *head_tmp = nullptr;                 // [rows][max ks * in_base]: a Conv1D head layer's input gradient before it is folded back over the taps
    float* ones = nullptr;    // [B * 2048] of 1.0: the GRU dropout masks are launch_dropout of it
    uint64_t dropout_seed = 0x5e1d5e1d5e1d5e1dull; unsigned dropout_step = 0, dropout_cur = 0; int last_training = 0;   // dropout_cur: the counter the LAST training forward drew its masks with (its backward recomputes them)
    float *loss_scratch = nullptr, *den_dev = nullptr, *loss_out = nullptr;
    float *fin_sl = nullptr, *fin_dl = nullptr;   // deferred loss finalize of the running training step
    int fin_doa_loss = 0;
    // trainv2 (trainv2.hip): device tables of the regulariser + AGC + AdaBelief stage, built once by seld_create from `tr` — column tiles of the
    // unit-norm kernel, segments of the update kernel, one regularised flag per variable (seld_set_regularized), one clip factor per unit
    struct V2Tab { void *tiles = nullptr, *segs = nullptr; int32_t* reg = nullptr; float* scale = nullptr; int ntiles = 0, nsegs = 0; } v2;
    float *swa_w = nullptr, *swa_s = nullptr;     // stochastic weight averaging (seld_swa_update): running means of params / state, allocated on first use
    int swa_cnt = 0;
    std::vector<void*> allocs;
    std::string err;
    int prof = 0;   // 0 off, 1 major kernel groups, 2 every group
    std::vector<Timer> timers;
    std::vector<hipEvent_t> ev_pool;   // timing events are created once and recycled: no hipEventCreate inside a timed step
};

// ---- errors, allocation (api.hip)
int fail(seld_ctx* c, int code, const std::string& msg);      // records msg on the context (c == nullptr: for seld_last_error(nullptr)), returns code
int check_launch(seld_ctx* c, const char* what);

#define HIPCHK(c, expr)                                                                         \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return fail(c, SELD_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));    \
    } while (0)

template <typename T>
int dalloc(seld_ctx* c, T** p, size_t n) {
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, n * sizeof(T) + 256);
    if (e != hipSuccess) return fail(c, SELD_ERR_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
    c->allocs.push_back(q);
    *p = reinterpret_cast<T*>(q);
    return 0;
}

// ---- profiling scopes
struct ProfScope {
    seld_ctx* c; int idx;
    ProfScope(seld_ctx* c_, const char* name, int level = 1) : c(c_), idx(-1) {
        if (c->prof < level) return;
        for (size_t i = 0; i < c->timers.size(); ++i) if (c->timers[i].name == name) idx = (int)i;
        if (idx < 0) { Timer t; t.name = name; c->timers.push_back(t); idx = (int)c->timers.size() - 1; }
        hipEvent_t e = take(c); hipEventRecord(e, c->stream); c->timers[idx].ev.push_back(e);
    }
    ~ProfScope() {
        if (idx < 0) return;
        hipEvent_t e = take(c); hipEventRecord(e, c->stream); c->timers[idx].ev.push_back(e);
        c->timers[idx].launches++;
    }
    static hipEvent_t take(seld_ctx* c) {
        if (c->ev_pool.empty()) { hipEvent_t e; hipEventCreate(&e); return e; }
        hipEvent_t e = c->ev_pool.back(); c->ev_pool.pop_back(); return e;
    }
};
#define PROF_CAT2(a, b) a##b
#define PROF_CAT(a, b) PROF_CAT2(a, b)
#define PROF(c, name) ProfScope PROF_CAT(prof_scope_, __LINE__)(c, name, 1)
#define PROF2(c, name) ProfScope PROF_CAT(prof_scope_, __LINE__)(c, name, 2)
// level 3: per-kernel-kind scopes INSIDE the level-1 groups of the block models (hundreds of event pairs per step: a separate
// profile pass of bench.py, never the pass that is timed for `value`)
#define PROF3(c, name) ProfScope PROF_CAT(prof_scope_, __LINE__)(c, name, 3)

// ---- shared by the passes (api.hip)
// side stream: everything enqueued on it after this call starts once the main stream has reached this point
void fork_side(seld_ctx* c);
// which path a context takes (the forward pass, its backward pass and the loss gradients must agree)
bool gru_sb(const seld_ctx* c, const GruL& G);
bool heads_general(const seld_ctx* c);
bool heads_sb(const seld_ctx* c);
bool heads_lin(const seld_ctx* c);
bool rn_c1_implicit(const seld_ctx* c, const RnBlock& R);
int rn_c1_width(const RnBlock& R);
bool rn_c1_direct(const RnBlock& R);

// ---- the passes (forward.hip, backward.hip)
int forward_impl(seld_ctx* c, const float* x, float* sed, float* doa, int training, bool save);
int backward_impl(seld_ctx* c, const float* x);

// ---- trainv2 (trainv2.hip): the v2 optimizer stage's device tables, at the end of seld_create
int v2_tables_create(seld_ctx* c);

// ---- data parallelism (dp.hip)
// in-place SUM over the ranks of the library's communicator; 0 = enqueued
int dp_allreduce(seld_ctx* c, void* buf, int64_t count, int dtype, hipStream_t st);
