/* seld_hip.h — C ABI of libseld_hip.so, the MI355X (gfx950) SELDnet hot path.
 *
 * The reference (IRIS-AUDIO/SELD) has no FFI; its seam is Python duck typing.  Every entry
 * point below names the reference interface it replaces (file:line under the reference tree).
 * The Python package `seld_amd` binds these with ctypes and mirrors the reference's
 * models.seldnet / train.trainstep / train.teststep surface on top of them.
 *
 * Conventions
 *  - every call returns int: 0 = ok, <0 = error (SELD_ERR_*); seld_last_error() has the text;
 *    no exception crosses the ABI.
 *  - pointers are DEVICE pointers unless the name ends in _host.  fp32 everywhere on the ABI.
 *  - the ctx owns weights, gradients, Adam slots, BN moving statistics and all workspace
 *    (sized at seld_create for a fixed [B,T,F,C]); the caller owns x / labels / outputs.
 *  - work is enqueued on the ctx's stream (default: the null stream; seld_set_stream to change)
 *    and is asynchronous; seld_sync() waits.  Calls on one ctx are not thread-safe; distinct
 *    ctxs are independent (one ctx per GPU / rank).
 *  - layouts are the reference's: x [B,T,F,C] (NHWC, H=time), conv kernels HWIO, GRU kernels
 *    [in,3u] gate order z|r|h with bias [2,3u], labels sed [B,S,nc], doa [B,S,3nc] as x|y|z blocks.
 */
#ifndef SELD_HIP_H
#define SELD_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define SELD_OK 0
#define SELD_ERR_INVALID (-1)     /* bad argument */
#define SELD_ERR_UNSUPPORTED (-2) /* valid config this build has no kernel for */
#define SELD_ERR_HIP (-3)         /* HIP runtime error */
#define SELD_ERR_NOMEM (-4)

#define SELD_DTYPE_F32 0
/* BASELINE.json configs[1]'s literal "bf16": every dense product of the step that has a single-product kernel (the three conv blocks'
 * forward / input gradient / kernel gradient, the GRU input projections and their input and kernel gradients) takes ONE bf16 MFMA product
 * with both operands rounded to nearest-even bf16 and fp32 accumulation, instead of the six products of the exact 3-way split that
 * SELD_DTYPE_F32 uses; tensors, BatchNorm statistics, the GRU recurrence, losses and Adam stay fp32.  Not within north_star's 1e-4: the
 * measured distance from the fp64 oracle is documented in DESIGN.md (outputs ~1e-3, gradients ~1e-2 of a variable's maximum).  The same
 * switch at run time: seld_set_option(ctx, "bf16_single", 0 | 1).  (2: SELD_DTYPE_F64 = 1 names the SyncBN callback's buffer type.) */
#define SELD_DTYPE_BF16 2

#define SELD_DOA_MSE 0  /* tf.keras.losses.MSE function form (train.py:317-320): [B,S] rows, tape sums them */
#define SELD_DOA_MMSE 1 /* losses.MMSE (losses.py:4-13) */
#define SELD_DOA_MAE 2  /* tf.keras.losses.MAE function form (params.py:16-17 choice 'MAE', train.py:317-318) */
#define SELD_DOA_MSLE 3 /* tf.keras.losses.MSLE function form (choice 'MSLE'): mean((log(max(p,1e-7)+1) - log(max(y,1e-7)+1))^2) */

#define SELD_MAX_LAYERS 4

typedef struct seld_ctx seld_ctx;

/* Architecture = what models.seldnet (models.py:18-32) reads from model_config/seldnet.json. */
typedef struct seld_arch {
    int32_t in_ch;                      /* C: 7 (foa) */
    int32_t n_freq;                     /* F: 64 */
    int32_t n_conv;                     /* len(FIRST_ARGS.filters) */
    int32_t filters[SELD_MAX_LAYERS];
    int32_t pool_t[SELD_MAX_LAYERS];    /* FIRST_ARGS.pool_size[i][0] */
    int32_t pool_f[SELD_MAX_LAYERS];    /* FIRST_ARGS.pool_size[i][1] */
    int32_t n_gru;                      /* len(SECOND_ARGS.units) */
    int32_t gru_units[SELD_MAX_LAYERS];
    int32_t n_sed_dense;                /* len(SED_ARGS.units) */
    int32_t sed_units[SELD_MAX_LAYERS];
    int32_t n_doa_dense;
    int32_t doa_units[SELD_MAX_LAYERS];
    int32_t n_classes;                  /* 12 (train.py:306-307) */
    /* FIRST block kind (models.py:24 getattr(modules, model_config['FIRST'])): 0 = simple_conv_block (filters / pool_* above),
     * 1 = xception_block (model_config/xception_gru.json; spec/XCEPTION_BLOCK.md): n_conv = 1 entry conv2d_bn(filters[0] = 2 x
     * FIRST_ARGS.filters) with pool (5,4), then xc_blocks = FIRST_ARGS.block_num residual modules of three
     * SeparableConv2D + BatchNormalization, then ReLU + MaxPooling2D((1,8)). */
    int32_t first_kind;
    int32_t xc_blocks;
    /* 2 = resnet50_block (model_config/resnet50_gru.json; spec/RESNET50_BLOCK.md): the same entry, then four stages of rn_blocks[s]
     * bottleneck blocks of width rn_filters * 2^s, frequency stride 2 at the first block of stages 1..3 -> [B, T/5, 2, 32 rn_filters] */
    int32_t rn_filters;
    int32_t rn_blocks[4];
    /* simple_dense_block's `dense_activation` (modules.py:356, 368-371): the activation of the heads' HIDDEN Conv1D layers (the output
     * Dense layers keep sigmoid / tanh, models.py:28-30).  0 = None / 'linear' (seldnet.json; lets W1 W2 fold into one product),
     * SELD_ACT_SIGMOID, SELD_ACT_TANH, SELD_ACT_RELU. */
    int32_t sed_dense_act;
    int32_t doa_dense_act;
    /* simple_dense_block's `kernel_size` (modules.py:355, 370-372: Conv1D(units, kernel_size, padding='same') over the frames of a clip;
     * 0 or 1 = per-step, seldnet.json) and `dropout_rate` (modules.py:357, 373-374: Dropout after every hidden layer, training only) of the
     * two heads.  The dropout masks are a counter-based function of (option "dropout_seed", the training step counter, layer, element):
     * see loss_adam.hip::dropout_kernel; TensorFlow's generator cannot be reproduced by another program. */
    int32_t sed_kernel_size;
    int32_t doa_kernel_size;
    float sed_dropout;
    float doa_dropout;
    /* 1 = models.seldnet_v1 (models.py:36-52; model_config/seldnet_v1.json): doa_out = tanh(doa * Concatenate([sed] * 3)). */
    int32_t output_coupling;
    /* `dropout_rate` of the FIRST and SECOND blocks (0 in every shipped config), training only; masks drawn like the heads' (dropout_kernel).
     * conv_dropout: simple_conv_block's Dropout(rate) behind every MaxPooling2D (model_config/seldnet.json:7; first_kind 0 only).
     * gru_dropout: bidirectional_GRU_block passes it as BOTH `dropout` and `recurrent_dropout` of every GRU (modules.py:306, 312-314): per
     * direction one input mask [B, in_feat] and one state mask [B, units], values 0 | 1/(1-rate), constant over the sequence (Keras GRUCell,
     * implementation 2: the input is masked before the kernel product, the previous state before the recurrent product AND the blend). */
    float conv_dropout;
    float gru_dropout;
} seld_arch;
#define SELD_ACT_NONE 0
#define SELD_ACT_SIGMOID 1
#define SELD_ACT_TANH 2
#define SELD_ACT_RELU 3
/* sizeof(seld_arch), sizeof(seld_loss_cfg) as the LIBRARY was compiled, into out[0..min(n,2)); returns how many it knows (2).  A binding
 * compares them with its own struct declarations before the first seld_create. */
int seld_abi_sizes(int32_t* out, int n);
#define SELD_FIRST_SIMPLE_CONV 0
#define SELD_FIRST_XCEPTION 1
#define SELD_FIRST_RESNET50 2
#define SELD_MAX_XC_BLOCKS 16

/* Loss configuration = train.py:311-320 + the `loss_weight` flag (params.py:30). */
typedef struct seld_loss_cfg {
    int32_t doa_loss;        /* SELD_DOA_MSE | SELD_DOA_MMSE | SELD_DOA_MAE | SELD_DOA_MSLE */
    float w_sed, w_doa;      /* loss_weight "1,1000" */
    float sed_grad_scale;    /* 1 on a single device; 1/world for data parallel MMSE runs */
    float mmse_den;          /* <=0: sum(mask) of this batch; >0: all-reduced global denominator */
} seld_loss_cfg;

/* ---- lifecycle: replaces getattr(models, 'seldnet')(input_shape, model_config) (train.py:308) */
int seld_create(const seld_arch* arch, int B, int T, int dtype, int device, seld_ctx** out);
void seld_destroy(seld_ctx* ctx);
const char* seld_last_error(const seld_ctx* ctx); /* ctx may be NULL: last create() error */
int seld_set_stream(seld_ctx* ctx, void* hip_stream);
/* batch size of the next calls, 1 <= B <= the B given to seld_create (the reference's Keras model
 * accepts any batch; data_loader.batch(drop_remainder=False) yields a short last batch) */
int seld_set_batch(seld_ctx* ctx, int B);
int seld_sync(seld_ctx* ctx);
/* compute options.  "conv64_split_bf16" (default 1): conv2/conv3 forward and input gradient run on the bf16 matrix
 * cores with every fp32 operand split exactly into three bf16 values and six partial products (fp32-level accuracy);
 * 0 selects the f32-input MFMA kernels.  "gemm_split_bf16" (default 1): the same scheme for the GRU input projections,
 * the heads' first Conv1D and their input gradients (gemm_sb.hip) where K % 32 == 0 and N % 128 == 0; 0 keeps them on
 * the f32-input MFMA GEMM.  "conv1_split_bf16" (default 1): the same scheme for the first
 * block's forward whenever its pre-BN tensor is not stored (conv_pool_sb.hip).  "conv1_pingpong" (default 1): that kernel for 7 input channels as one
 * 8-wave workgroup per CU whose two wave groups alternate matrix and vector segments (the same bits; 0: the 4-wave kernel, which 10 channels
 * always take).  "conv1_pool_fused" / "conv1_gram" (default 1): first block's pooling inside the conv
 * epilogue / its kernel gradient from the patch Gram matrix.  "dropout_seed" / "dropout_step" (values): the key of the heads' dropout
 * draws and the step counter of the next training forward (seld_arch.sed_dropout / doa_dropout; INTEGRATION.md section 6 lists every key).
 * EVERY key is per context: the kernel choices ("bwd_four_products", "dgrad_r8", "conv1_pingpong", "tn_tile_blocks", "gram_bg_blocks",
 * "bf16_single", ...) are stored in the context and handed to every kernel launch of its passes as an argument, so a six-product
 * context and a four-product context coexist in one process, from one host thread or from two
 * (calls on one context are not thread-safe). */
int seld_set_option(seld_ctx* ctx, const char* key, int value);

/* ---- variables: replaces model.trainable_variables / get_weights / set_weights
 * (train.py:31-34, evaluator.py:57).  Flat fp32, Keras creation order; seld_variable_info
 * enumerates (name, offset, shape).  "state" = BN moving_mean/moving_variance pairs. */
int64_t seld_param_count(const seld_ctx* ctx);
int64_t seld_state_count(const seld_ctx* ctx);
int seld_variable_count(const seld_ctx* ctx, int trainable);
int seld_variable_info(const seld_ctx* ctx, int trainable, int index, char* name, int name_cap,
                       int64_t* offset, int32_t* rank, int64_t shape[4]);
int seld_set_weights_host(seld_ctx* ctx, const float* w_host, int64_t n);
int seld_get_weights_host(seld_ctx* ctx, float* w_host, int64_t n);
int seld_set_state_host(seld_ctx* ctx, const float* s_host, int64_t n);
int seld_get_state_host(seld_ctx* ctx, float* s_host, int64_t n);
int seld_get_grads_host(seld_ctx* ctx, float* g_host, int64_t n);
int seld_get_adam_host(seld_ctx* ctx, float* m_host, float* v_host, int64_t n);
int seld_set_adam_host(seld_ctx* ctx, const float* m_host, const float* v_host, int64_t n, int64_t step);
void* seld_param_ptr(seld_ctx* ctx); /* device, [param_count] fp32 */
void* seld_grad_ptr(seld_ctx* ctx);  /* device, [param_count] fp32: the DP all-reduce buffer */

/* ---- model(x, training) (models.py:18-32; train.py:25,41).  training!=0: batch statistics,
 * moving statistics updated.  sed [B,S,nc], doa [B,S,3nc], S = T / prod(pool_t). */
int seld_forward(seld_ctx* ctx, const float* x, float* sed, float* doa, int training);

/* Data-parallel overlap: after seld_train_fwd_bwd has been ENQUEUED, make `stream` wait until the gradients of the
 * GRU and head variables — grads[*offset : param_count), 86 % of the buffer — are final.  They are produced on the
 * library's side stream early in the backward pass, so a host can start their all-reduce on a communication stream
 * while the conv backward is still running on the main stream; grads[0 : *offset) (conv/BN) are final when the main
 * stream has drained.  (No counterpart in the reference, which has no distributed path.) */
int seld_grads_tail_ready(seld_ctx* ctx, void* stream, int64_t* offset);
/* The same hand-off at the granularity the backward pass produces gradients in: bucket 0 = the last GRU layer + the heads
 * (final when that layer's BPTT has run and its weight-gradient GEMMs have drained on the side stream, i.e. while the earlier
 * layers' recurrences are still running), bucket k = GRU layer n_gru-1-k, the last bucket = the conv/BN variables (final when
 * the main stream has drained).  seld_grads_bucket_ready makes `stream` wait for bucket `index` of the last ENQUEUED
 * seld_train_fwd_bwd and returns its [offset, offset + count) range of the flat gradient buffer. */
int seld_grads_bucket_count(const seld_ctx* ctx);
int seld_grads_bucket_ready(seld_ctx* ctx, int index, void* stream, int64_t* offset, int64_t* count);
/* ---- synchronised BatchNorm for data parallelism (a B/world-per-rank run then equals the reference's
 * single-device batch, layers.py:33 with params.py:27's batch of 256).  The library calls `fn(user, buf, count, dtype, stream)`
 * — dtype SELD_DTYPE_F64, count 128 * ceil(C / 64) + 1 = [sum z | sum z^2] resp. [sum dy | sum dy xhat] per channel (128 for the 64-channel
 * blocks, up to 2048 for resnet50_block's 1024-channel BatchNormalizations) followed by THIS rank's element count (so ranks may hold
 * different numbers of clips: the global count is the all-reduced one) — once per BatchNormalization in the
 * training forward and once in the backward; fn must enqueue an in-place SUM over the `world` ranks of the device buffer `buf`
 * on `stream` (e.g. ncclAllReduce / torch.distributed.all_reduce) and return 0.  fn == NULL switches back to per-replica
 * statistics.  dgamma / dbeta stay per-rank partial sums like every other gradient (the gradient all-reduce completes them). */
#define SELD_DTYPE_F64 1
typedef int (*seld_allreduce_fn)(void* user, void* buf, int64_t count, int dtype, void* hip_stream);
int seld_set_sync_bn(seld_ctx* ctx, seld_allreduce_fn fn, void* user, int world);
/* ---- data parallelism INSIDE the library: one process per GPU, a full weight replica per rank, the
 * batch sharded by clips; the reference has no counterpart (train.py:22-36 is single device).  The library owns an RCCL communicator
 * (RCCL is bound with dlopen at the first seld_dp_* call: no link-time dependency), a communication stream and the bucket order.
 *   seld_dp_available()              : 1 if RCCL could be bound in this process, else 0 — what every rank OTHER than 0 calls before the
 *                                      host's agreement step (ncclGetUniqueId starts a bootstrap listener: only rank 0 draws an id)
 *   seld_dp_unique_id(id)            : rank 0 fills 128 bytes (ncclUniqueId); the host carries them to every rank by its own means
 *   seld_dp_init(ctx, rank, world, id): ncclCommInitRank on the ctx's device (collective: every rank calls it)
 *   seld_dp_allreduce_grads(ctx)     : between seld_train_fwd_bwd and seld_adam_step — TWO in-place ncclAllReduce(SUM) over the flat
 *                                      gradient buffer: GRU + heads as soon as those gradients are final (the conv backward is still
 *                                      running), then the conv / BN variables; the ctx stream waits for both
 *   seld_dp_set_sync_bn(ctx, on)     : synchronised BatchNorm (see seld_set_sync_bn) through the same communicator
 *   MMSE loss: with a communicator and cfg.mmse_den <= 0 the mask count is all-reduced on the device inside seld_train_fwd_bwd /
 *              seld_test_step; the caller sets cfg.sed_grad_scale = 1 / world (loss-reduction rules: DESIGN.md section 5)
 * A failed collective is fatal for the process group: peers block in theirs — abort the job. */
int seld_dp_available(void);
int seld_dp_unique_id(void* id_out_128_bytes);
int seld_dp_init(seld_ctx* ctx, int rank, int world, const void* unique_id_128_bytes);
int seld_dp_world(const seld_ctx* ctx);
int seld_dp_allreduce_grads(seld_ctx* ctx);
int seld_dp_set_sync_bn(seld_ctx* ctx, int on);
int seld_dp_destroy(seld_ctx* ctx);
/* ---- train.trainstep (train.py:22-36), split so that a data-parallel host can all-reduce
 * seld_grad_ptr() between the two halves:
 *   seld_train_fwd_bwd : forward(training=True) + losses + tape.gradient -> grad buffer
 *   seld_adam_step     : optional AGC (utils.py:86-96) + Adam.apply_gradients (Keras Adam, eps 1e-7)
 * sloss: 1 float; dloss: [B*S] floats (MSE) or 1 float (MMSE); either may be NULL. */
int seld_train_fwd_bwd(seld_ctx* ctx, const float* x, const float* y_sed, const float* y_doa,
                       const seld_loss_cfg* cfg, float* sed, float* doa, float* sloss, float* dloss);
int seld_adam_step(seld_ctx* ctx, float lr, float beta1, float beta2, float eps, int agc);
int seld_train_step(seld_ctx* ctx, const float* x, const float* y_sed, const float* y_doa,
                    const seld_loss_cfg* cfg, float lr, int agc, float* sed, float* doa,
                    float* sloss, float* dloss);
/* ---- train.teststep (train.py:39-44) */
int seld_test_step(seld_ctx* ctx, const float* x, const float* y_sed, const float* y_doa,
                   const seld_loss_cfg* cfg, float* sed, float* doa, float* sloss, float* dloss);
/* sum(mask) of losses.MMSE for this batch (1 float, device) — for the DP denominator all-reduce */
int seld_mmse_den(seld_ctx* ctx, const float* y_doa, float* den);

/* ---- the step of the reference's second training script (trainv2.py:23-56; DESIGN.md "The trainv2 recipe"): class-weighted BCE or
 * focal loss with optional label smoothing, losses.MMSE_with_cls_weights, an L2 kernel regulariser, AGC on every step, AdaBelief, and
 * stochastic weight averaging.  Purely additive: train.py's entry points above are unchanged. */
#define SELD_SED_BCE 0   /* mean(K.binary_crossentropy(t, p) * cls_weights) (trainv2.py:41, :293) */
#define SELD_SED_FOCAL 1 /* mean(losses.focal_loss(t, p) * cls_weights) = focal * mean(cls_weights) (losses.py:29-34: the loss is a scalar) */
#define SELD_V2_MAX_CLASSES 32
typedef struct seld_v2_cfg {
    int32_t sed_loss;                         /* SELD_SED_BCE | SELD_SED_FOCAL */
    float w_sed, w_doa;                       /* loss_weights */
    float label_smoothing;                    /* [0, 1): t = y (1 - ls) + 0.5 ls when > 0 (trainv2.py:38-39) */
    float focal_alpha, focal_gamma;           /* losses.focal_loss defaults: 0.25, 2 */
    float cls_weights[SELD_V2_MAX_CLASSES];   /* the first n_classes are read (trainv2.py:25-30: mean(train_samples) / train_samples) */
} seld_v2_cfg;
/* seld_train_fwd_bwd with the v2 loss stage: objective = sloss w_sed + dloss w_doa, both scalars (sloss, dloss: 1 float each, may be
 * NULL).  The weighted MMSE denominator is computed on the device from the labels.  SELD_ERR_INVALID, before anything is enqueued, for a
 * NULL required pointer, n_classes > SELD_V2_MAX_CLASSES, an unknown sed_loss or label_smoothing outside [0, 1); SELD_ERR_UNSUPPORTED on a
 * context with a data-parallel communicator (the reference defines no weighted denominator / loss scaling across ranks). */
int seld_train_fwd_bwd_v2(seld_ctx* ctx, const float* x, const float* y_sed, const float* y_doa, const seld_v2_cfg* cfg, float* sed,
                          float* doa, float* sloss, float* dloss);
/* utils.apply_kernel_regularizer (utils.py:343-350): flags[i] != 0 marks trainable variable i (seld_variable_info order) as carrying the L2
 * term l2 sum(w^2) in the objective.  Default: none.  SELD_ERR_INVALID unless n_trainable_variables == seld_variable_count(ctx, 1). */
int seld_set_regularized(seld_ctx* ctx, const int32_t* flags, int n_trainable_variables);
/* The optimizer stage of trainv2.trainstep in two launches, whatever the number of variables: g' = (g + 2 l2 w flag) * clip, the clip of
 * utils.adaptive_clip_grad (utils.py:86-96; clip_factor 0.01 in the reference, <= 0: no clipping) per unit on the regularised gradient; then
 * utils.AdaBelief (utils.py:157-182, amsgrad=False): m = b1 m + (1 - b1) g', v = b2 v + (1 - b2) (g' - m)^2 with the UPDATED m,
 * w -= lr sqrt(1 - b2^t) / (1 - b1^t) m / (sqrt(v) + eps).  The moments are the context's Adam slots (seld_get_adam_host / seld_set_adam_host
 * serve both optimizers); g' is written back to the gradient buffer. */
int seld_v2_opt_step(seld_ctx* ctx, float lr, float beta1, float beta2, float eps, float l2, float clip_factor);
/* swa.SWA (swa.py:25-32) over the weights AND the BatchNorm moving statistics (model.get_weights() holds both): update folds the current
 * values into the running mean swa = (swa cnt + w) / (cnt + 1) in fp32 (the first update copies; buffers are allocated then); count = the
 * number of updates so far; apply = on_train_end's model.set_weights(swa_weights) — SELD_ERR_INVALID before the first update. */
int seld_swa_update(seld_ctx* ctx);
int seld_swa_count(const seld_ctx* ctx);
int seld_swa_apply(seld_ctx* ctx);

/* ---- feature stage: replaces feature_extractor.extract_features (feature_extractor.py:53-88) and, for the
 * in-loop variant, apply_normalizer + preprocess_features_labels (:117-149, :226-234).
 * complex_spec (:153-173) = torchaudio spectrogram(hann(win_length) periodic, n_fft, hop, power=None, center, reflect);
 * mode 0 'foa': 4 log-mel (top_db 80 over the clip) + 3 mel intensity vectors; mode 1 'mic': 4 log-mel + 6 GCC-PHAT.
 * wav [4][n_samples] fp32 (device) -> out [1 + n_samples/hop][n_mels][7|10] fp32 (device), the reference's
 * [time, freq, chan] layout.  `stream` is a hipStream_t (NULL = null stream). */
typedef struct seld_feat seld_feat;
int seld_feat_create(int sample_rate, int n_fft, int win_length, int hop_length, int n_mels, int mode, int normalized,
                     int device, seld_feat** out);
void seld_feat_destroy(seld_feat* f);
const char* seld_feat_last_error(const seld_feat* f);
/* kernel selection, for A/B runs and parity of the fallback: "wave_kernel" (default 1): one wave per frame with a radix-4 FFT
 * in registers + LDS (n_fft 256 .. 1024); 0: the workgroup-per-frame radix-2 kernel that serves every other n_fft */
int seld_feat_set_option(seld_feat* f, const char* key, int value);
int64_t seld_feat_frames(const seld_feat* f, int64_t n_samples);
int seld_feat_channels(const seld_feat* f);
int seld_feat_extract(seld_feat* f, const float* wav, int n_ch, int64_t n_samples, float* out, void* stream);
/* The same for `n_clips` clips of ONE length in one pair of launches (what a data loader preprocessing a list of equal-length files,
 * feature_extractor.py:238-262, does clip by clip): wav [n_clips][n_ch][n_samples] -> out [n_clips][frames][n_mels][7|10]; the
 * top_db clamp stays per clip.  Launch overheads and the tail of a 3 001-frame grid amortise over the batch. */
int seld_feat_extract_batch(seld_feat* f, const float* wav, int n_clips, int n_ch, int64_t n_samples, float* out, void* stream);
/* (x - mean)/max(std, eps) per (freq, chan), rows trimmed / zero-padded (before normalising, as the reference does) to T_out */
int seld_feat_normalize(const float* feat, const float* mean, const float* stdv, float* out, int64_t T_in, int64_t T_out,
                        int FC, float eps, void* stream);
/* calculate_statistics (feature_extractor.py:218-224): per-(freq, chan) mean and population std over ALL frames of a list of feature
 * tensors.  `acc` = 2*FC + 1 doubles on the device (sum | sum of squares | row count; zero it to start), folded once per tensor
 * feat [rows][FC] (any number of calls, any row counts: a file, or a batch [n][T][FC] as n*T rows); `scratch` =
 * seld_feat_stats_scratch_doubles(FC) doubles (device).  Fixed-order double sums: bit-reproducible for a given call sequence.
 * seld_feat_stats_finalize writes float mean / std [FC] (the reference's [1, freq, chan] arrays). */
int64_t seld_feat_stats_scratch_doubles(int FC);
int seld_feat_stats_accumulate(const float* feat, int64_t rows, int FC, double* acc, double* scratch, void* stream);
int seld_feat_stats_finalize(const double* acc, int FC, float* mean, float* stdv, void* stream);

/* ---- sliding-window inference: the two tensor ops around model() in evaluator.ensemble_outputs
 * (evaluator.py:16-50, trainv2.py:158-192).
 * seld_frame_windows: tf.signal.frame(x [T,FC], win_size, step, axis=0)[first_window : first_window+n_windows]
 *                     -> windows [n_windows, win_size, FC]   (FC = freq*chan, multiple of 4)
 * seld_overlap_average: tf.signal.overlap_and_add(y [n_windows, L, D], frame_step=1) / window count -> [n_windows-1+L, D] */
int seld_frame_windows(const float* x, float* windows, int T, int FC, int win_size, int step, int first_window, int n_windows,
                       void* stream);
int seld_overlap_average(const float* y, float* out, int n_windows, int L, int D, void* stream);

/* ---- batch augmentation on the device (reference: the tf.data sample/batch transforms of train.get_dataset,
 * train.py:157-165).  The random draws are made by the host (seld_amd/transforms.py mirrors the reference's
 * distributions) and passed as small device arrays; the kernels are pure data movement.
 * seld_aug_mask: transforms.mask (transforms.py:6-44) for both axes in one pass over x [B,T,F,C], in place: for sample
 *   b and segment s = t / period (T % period == 0, else SELD_ERR_INVALID as the reference raises ValueError), frames
 *   [t_off, t_off+t_size) of the segment and bins [f_off, f_off+f_size) are zeroed; arrays are int32 [B * T/period];
 *   either pair may be NULL (that axis is not masked).
 * seld_aug_gather_sign: out[b,o,r,i] = sgn[b,r] * in[b,o,src[b,r],i] in place on x [B,outer,R,inner] (R <= 32): the
 *   channel permutation + sign flips of foa_intensity_vec_aug / acs_aug (transforms.py:73-114,159-207) on the
 *   features (R = channels, inner = 1) and on the labels viewed [B,S,4,n_classes] (R = 4, inner = n_classes). */
int seld_aug_mask(float* x, int B, int T, int F, int C, int period, const int* t_off, const int* t_size, const int* f_off,
                  const int* f_size, void* stream);
int seld_aug_gather_sign(float* x, int B, int64_t outer, int R, int64_t inner, const int* src, const float* sgn, void* stream);
/* seld_aug_v2: the sample transforms of trainv2.get_dataset (trainv2.py:120-140) in ONE pass over x [B,T,F,C], in place: shift[b] is
 *   added to the channels < n_shift_ch (random_ups_and_downs; shift float [B], may be NULL), then, per sample and per `period`-frame
 *   segment, the union of n_t frame runs and the union of n_f bin runs is stored as +0.0f — the bits of the add followed by n_t + n_f
 *   seld_aug_mask calls.  Tables: int32 [n_t][B * T/period] and [n_f][B * T/period]; n_t / n_f may be 0 (that axis's pointers may then be
 *   NULL).  The four tables are read by the host, for the checks below, AND by the kernel: they must be host memory the device can read
 *   (hipHostMalloc / a pinned torch tensor), alive until the kernel has run; shift is read by the kernel only.  Asynchronous on `stream`,
 *   no allocation, no copy, no host synchronisation.  SELD_ERR_INVALID, before the first HIP call, for T % period != 0, n_t or n_f above
 *   16, n_shift_ch > C, a negative size or offset, or a run that reaches outside its axis (offset + size > period, or > F);
 *   SELD_ERR_UNSUPPORTED for F * C > 16384. */
int seld_aug_v2(float* x, int B, int T, int F, int C, int period, const float* shift, int n_shift_ch, const int* t_off, const int* t_size,
                int n_t, const int* f_off, const int* f_size, int n_f, void* stream);
/* seld_aug_mcs: transforms.mcs_aug (transforms.py:202-291, with its tf_cond / is_invertible / stab helpers), the CGMM mask estimator, in
 *   ONE launch over x [B,T,F,C] float32: per (b, f) column, in float64, the covariance initialisation, `iteration` EM rounds and
 *   out[b,t,f,:] = x[b,t,f,:] * float32(lambda_noise[b,t,f]) of the last round (the product in fp32).  `out` may be x itself (in place); any
 *   other overlap is the caller's error.  lambda (nullable) receives lambda_noise as [B,T,F] doubles; stab_adds (nullable) receives, as
 *   int32 [B,F,2,iteration+1], the number of diagonal additions (0..6) of every stab call: class noisy then class noise, the
 *   initialisation's call first.  Fixed summation order, no atomics: two calls give the same bits.  Asynchronous on `stream`, no allocation,
 *   no host synchronisation.  Before anything is enqueued: SELD_ERR_INVALID for a NULL x or out, B, T or F < 1, iteration < 1 (the
 *   reference's function has no result there), a theta that is negative or not finite; SELD_ERR_UNSUPPORTED for C outside 1..10 and for
 *   T > seld_aug_mcs_max_frames(C).  Non-finite inputs are outside the contract: that column's output is unspecified.
 * seld_aug_mcs_max_frames: the largest T the kernel holds on chip for this C (>= 3000 for every C <= 10); 0 for an unsupported C. */
int seld_aug_mcs_max_frames(int C);
int seld_aug_mcs(const float* x, float* out, double* lambda, int32_t* stab_adds, int B, int T, int F, int C, int iteration, double theta,
                 void* stream);
/* Time-domain mixing: data_loader.TDM_aug (data_loader.py:188-234), which train.get_tdm_dataset (train.py:210-261) runs on the host over the
 *   whole training split every --tdm_epoch epochs (train.py:279-288, 341-356).  The host makes the reference's draws and passes them as a plan,
 *   int32 [B][K][4] = (cls, st, offset, td_offset) on the device (16-byte aligned): insertion k of a clip adds `st` label frames of bank class
 *   `cls`, from frame td_offset of that class's track, at label frame `offset` of the clip.  nc = W / 4; a label row is [activity | x | y | z].
 *   Both calls are asynchronous on `stream`: no allocation, no copy, no host synchronisation, no atomics, fixed order (the same bits every call).
 * seld_aug_tdm_labels: the labels, y [B][T][W] in place.  bank_y holds the classes' label tracks packed row-wise: class k is rows
 *   bank_row0[k] .. bank_row0[k] + bank_rows[k] of [W] floats (int64 [n_cls] each, device).  One workgroup per clip runs its K insertions in
 *   order: v[f] = (sum_{c<nc} y[off+f][c] < max_per_frame ? 1 : 0) * (1 - y[off+f][cls]) for f < st (sum over c ascending in fp32; fractional
 *   activities give a fractional v, as in the reference), then y[off+f][:] += bank_y[cls][td+f][:] * v[f] (multiply, then add).  valid, float
 *   [B][K][ld_valid], is WRITTEN: v[f] for f < st, 0 behind.  A plan row that reaches outside the clip, the class's track or ld_valid
 *   (cls outside [0, n_cls), st outside [1, min(T, ld_valid)], offset < 0, offset + st > T, td_offset < 0, td_offset + st > bank_rows[cls])
 *   is skipped and its valid row is 0: nothing outside a buffer is read.  The reference's early return when sum(v) == 0 adds zeros here.
 * seld_aug_tdm_mix: the waveforms, x_in -> x_out [B][C][N], N >= T * spf (spf = samples per label frame, 2400 in the reference); x_out == x_in
 *   is allowed (in place), any other overlap is the caller's error.  bank_x packing: class k's waveform is ONE block [C][n_k] of floats that
 *   starts at bank_x + bank_s0[k] (channel c at + c * n_k), the blocks one behind the other; bank_s0 is int64 [n_cls + 1] on the device, its
 *   last entry the end of the last block, so that n_k = (bank_s0[k+1] - bank_s0[k]) / C is known to the kernel, which skips a plan row with
 *   (td_offset + st) * spf > n_k.  `valid` is what seld_aug_tdm_labels wrote for this plan.  One workgroup per (clip, label frame) holds
 *   the frame's C x spf samples in registers and applies the insertions that cover it in plan order, x = x + t * v[f - offset] (multiply, then
 *   add: the bits of the reference's x[i] += pad(...) one insertion after the other); a frame no insertion covers is not touched in place and
 *   copied out of place, as are the samples at and behind T * spf.  float4 accesses when spf % 4 == 0, N % 4 == 0 and x_in, x_out and bank_x
 *   are 16-byte aligned (a class with bank_s0[k] % 4 != 0 or n_k % 4 != 0 is then read with scalar loads), else a scalar form.
 * Before anything is enqueued, both: SELD_ERR_INVALID for a NULL pointer, B, T, W, C, spf or n_cls < 1, W % 4 != 0, K < 0, ld_valid < 1,
 *   N < T * spf, a plan that is not 16-byte aligned, more bank classes than label classes (n_cls > W / 4); SELD_ERR_UNSUPPORTED for K > 32 and for more than 2^24 - 1 workgroups (B, or B * T).
 *   K == 0: SELD_OK, nothing enqueued (plan and valid may be NULL) — except the mix out of place, which still copies x_in to x_out. */
int seld_aug_tdm_labels(float* y, int B, int T, int W, const float* bank_y, const int64_t* bank_row0, const int64_t* bank_rows, int n_cls,
                        const int32_t* plan, int K, int max_per_frame, float* valid, int ld_valid, void* stream);
int seld_aug_tdm_mix(const float* x_in, float* x_out, int B, int C, int64_t N, int T, int spf, const float* bank_x, const int64_t* bank_s0,
                     int n_cls, const int32_t* plan, int K, const float* valid, int ld_valid, void* stream);

/* ---- SELD metrics on the device: SELDMetrics.update_states (metrics.py:60-154), which the reference runs in TF
 * eager mode on the host after every step (train.py:82-83).  `state` = seld_metrics_state_size(nc) doubles
 * (device, zero to reset): TP FP TN FN S D I Nref Nsys total_DE DE_TP, then class_tp|fp|tn|fn [nc] each;
 * `scratch` = seld_metrics_scratch_floats(...) floats (device).  y_true / y_pred = (sed [B,S,nc], doa [B,S,3nc]). */
int seld_metrics_state_size(int n_classes);
int64_t seld_metrics_scratch_floats(int B, int S, int n_classes, int block_size);
int seld_metrics_update(const float* sed_true, const float* doa_true, const float* sed_pred, const float* doa_pred, int B, int S,
                        int n_classes, int block_size, float doa_threshold, double* state, float* scratch, void* stream);

/* ---- the segment-based, location-aware DCASE score on the device: SELDMetrics_.update_seld_scores
 * (SELD_evaluation_metrics.py:63-154) with distance_between_cartesian_coordinates (:171-188), which trainv2.evaluate_fn
 * (trainv2.py:195-237) reaches per file through a csv file, nested dicts and a Hungarian assignment per (frame, class).
 * Inputs are concatenated over n_files files; file_off [n_files + 1] is a HOST array, file_off[0] = 0, strictly ascending,
 * N = file_off[n_files].  A block_size-frame segment never spans two files; a file's last segment may be ragged.
 *   sed [N, nc], doa [N, 3nc] fp32 (class c's vector: columns c, nc + c, 2nc + c); sed_thresh [nc] (active iff sed > thresh);
 *   gt_xyz [N, nc, K, 3] fp64; gt_slot [N, nc, K] uint8: dense index (< SELD_DCASE_MAX_SLOTS) of the entry's track id among the
 *   distinct ids of its (segment, class) in order of first appearance; gt_n [N, nc] int32 entries per (frame, class), 0..K.
 * `state` = seld_dcase_state_size() doubles (device, zero to reset): TP FP FN S D I Nref total_DE DE_TP DE_FP DE_FN; the call
 * adds to it.  `scratch` = seld_dcase_update_scratch_bytes(N, n_files, block_size) bytes (device, 8-byte aligned).  Two stages
 * in a fixed order, no atomics: equal inputs give equal bits.  SELD_ERR_INVALID before the first HIP call for a NULL pointer,
 * offsets that do not ascend from 0, nc < 1, K outside 1..SELD_DCASE_MAX_SLOTS, block_size outside 1..32, N nc > INT32_MAX.  The
 * segment table is built on the host and copied once; the call waits for that copy, then returns with the kernels enqueued. */
#define SELD_DCASE_MAX_SLOTS 8
int seld_dcase_state_size(void);
int64_t seld_dcase_update_scratch_bytes(int64_t N, int n_files, int block_size);
int seld_dcase_update(const float* sed, const float* doa, const float* sed_thresh, const double* gt_xyz, const uint8_t* gt_slot,
                      const int32_t* gt_n, const int32_t* file_off, int n_files, int n_classes, int K, int block_size, double doa_threshold,
                      double* state, void* scratch, void* stream);
/* the per-class threshold sweep: table [n_classes * n_cand + 1][11] doubles (device).  Row c * n_cand + k holds the eleven counters, in
 * seld_dcase_update's order, for the threshold vector base_thresh [nc] (device) with entry c replaced by cand[k] (cand [n_cand], device);
 * the last row is base_thresh itself.  The table is overwritten.  Every row has the bits seld_dcase_update leaves in a zeroed state
 * for that vector: the distances and the arg-min slots do not depend on a threshold and are computed once per (segment, class), and
 * total_DE is added in that call's order (classes, then slots, ascending within a segment; seld_dcase_update's reduction over the
 * segments).  Candidates may repeat and come in any order; active iff sed > threshold in fp32.  No atomics.  `scratch` =
 * seld_dcase_sweep_scratch_bytes(N, n_files, nc, n_cand, block_size) bytes (device, 8-byte aligned), linear in
 * segments * nc * (n_cand + 1).  The refusals and the one copy of seld_dcase_update, and SELD_ERR_INVALID (-1 from the scratch
 * function) for n_cand outside 1..SELD_DCASE_MAX_CAND or a NULL cand or table. */
#define SELD_DCASE_MAX_CAND 16
int64_t seld_dcase_sweep_scratch_bytes(int64_t N, int n_files, int n_classes, int n_cand, int block_size);
int seld_dcase_sweep(const float* sed, const float* doa, const float* base_thresh, const float* cand, const double* gt_xyz,
                     const uint8_t* gt_slot, const int32_t* gt_n, const int32_t* file_off, int n_files, int n_classes, int K, int n_cand,
                     int block_size, double doa_threshold, double* table, void* scratch, void* stream);
/* the tf.where + gather of utils.write_answer (utils.py:249-264) for every file at once: the active (frame-in-file, class) pairs in
 * row-major order, file after file, and class c's DOA vector beside each.  row_fc int32 [cap, 2], row_xyz fp32 [cap, 3] with
 * cap = N nc; row_off int32 [n_files + 1]: file f's rows are [row_off[f], row_off[f + 1]).  All three on the device.  `scratch` =
 * seld_answer_rows_scratch_bytes(N, n_files, nc) bytes.  An ordered compaction (count per chunk, scan, write) without atomics.  Same
 * refusals and the same one copy (file_off) as seld_dcase_update. */
int64_t seld_answer_rows_scratch_bytes(int64_t N, int n_files, int n_classes);
int seld_answer_rows(const float* sed, const float* doa, const float* sed_thresh, const int32_t* file_off, int n_files, int n_classes,
                     int32_t* row_fc, float* row_xyz, int32_t* row_off, void* scratch, void* stream);

/* ---- measurement: HIP-event timing of named kernel groups on the ctx stream (bench.py roofline).
 * seld_profile_enable(ctx, level): 0 off, 1 the largest groups (conv1 fwd / conv1 wgrad / GRU fwd / GRU BPTT, the resnet stages), 2 every group,
 * 3 additionally one scope per product / BatchNorm launch of resnet50_block (hundreds of event pairs per step: a profile pass, not a timed one) */
int seld_profile_enable(seld_ctx* ctx, int on);
int seld_profile_count(const seld_ctx* ctx);
int seld_profile_get(seld_ctx* ctx, int index, char* name, int name_cap, int64_t* launches, double* total_ms);
int seld_profile_reset(seld_ctx* ctx);

/* ---- per-kernel entry points (unit parity tests; all device pointers, null stream) --------
 * Each cites what it computes in the reference.  Shapes are checked; SELD_ERR_UNSUPPORTED if
 * the build has no kernel for them. */
/* same keys as seld_set_option, for the seld_k_* entry points: PROCESS-WIDE (there is no context).  Defaults: the product's
 * ("bwd_four_products" 1: the unit entry points' backward products also run on four of the six split terms).  A value holds until it is
 * set again: no context reads these and no context's pass changes them, so a caller that sets one restores it when done. */
int seld_k_set_option(const char* key, int value);
/* Conv2D(64, 3, padding='same', use_bias=True) on NHWC (layers.py:27-32); x [B,H,W,Cin], w HWIO, z [B,H,W,64].
 * stats (may be NULL): [2*64] = per-channel sum(z), sum(z^2) over B*H*W (BatchNormalization batch statistics). */
int seld_k_conv3x3_fwd(const float* x, const float* w, const float* bias, float* z, float* stats,
                       int B, int H, int W, int Cin, int Cout);
/* The same 64 -> 64 convolution with the previous block's BatchNormalization + ReLU applied while x is loaded (split-bf16 region kernel, W = 16 or 4):
 * x is the previous block's window-extreme tensor, a = max(0, fma(x, pre_scale[c], pre_shift[c])) the arithmetic of seld_k_bn_relu_ext,
 * z = conv(a) + bias and stats as in seld_k_conv3x3_fwd(a), bit for bit.  pre_out (may be NULL: inference) [B,H,W,64] receives a and must not be x.
 * ext_out (may be NULL; W = 16, needs ext_gamma [64]) [B,H,4,64]: per (1,4) window and channel the maximum of z where ext_gamma >= 0, the minimum
 * where ext_gamma < 0.  pre_scale == NULL: the plain convolution.  SELD_ERR_UNSUPPORTED wherever the launcher refuses (another width with pre_scale
 * or ext_out, ext_out without pre_scale or ext_gamma, pre_out == x, option "bf16_single" with pre_scale). */
int seld_k_conv3x3_fwd_pre(const float* x, const float* pre_scale, const float* pre_shift, const float* w, const float* bias, float* z, float* stats,
                           float* pre_out, const float* ext_gamma, float* ext_out, int B, int H, int W);
/* First conv block forward with the (5,4) MaxPooling2D reduction folded into the convolution (layers.py:27-37,
 * seldnet.json FIRST_ARGS pool_size[0]): x [B,H,64,Cin] (Cin 7 or 10, H % 5 == 0) -> z [B,H,64,64] (may be NULL:
 * not stored), zext [B,H/5,16,64] = per pooling window max(z) where gamma >= 0 / min(z) where gamma < 0, amax
 * [B,H/5,16,64] bytes = position row*4+col of that extreme inside its window (what MaxPoolGrad routes to; the first
 * in column-then-row scan order on ties; may be NULL only if z is NULL), and the batch statistics as in
 * seld_k_conv3x3_fwd.  BN+ReLU is monotone in z, so MaxPool(ReLU(BN(z))) == seld_k_bn_relu_ext(zext) bit for bit. */
int seld_k_conv_first_fwd_pool(const float* x, const float* w, const float* bias, const float* gamma, float* z, float* zext,
                               unsigned char* amax, float* stats, int B, int H, int Cin);
/* The first block trained WITHOUT its pre-BN tensor (conv_gram.hip): z = P W + b is linear in the im2col patches P, so
 * the kernel/bias gradient through BatchNorm(batch statistics)+ReLU+MaxPool(5,4) is
 *   dW = ka (G W + g b) + g kb + M,   G = P^T P (Gram matrix of the input patches), g = column sums of P,
 *   M[k][co] = sum over windows with p > 0 of scale[co] dp P[recorded argmax pixel][k]
 * seld_k_conv1_gram: G alone, [KP x KP] floats with KP = 64 (Cin 7) / 128 (Cin 10); row/column 9*Cin is the ones column
 *   (G[k][9 Cin] = g[k], G[9 Cin][9 Cin] = B*H*64); only the upper 32x32 tiles are written (symmetric).
 * seld_k_conv1_train_gram: the whole block from x: forward (window extremes, positions, statistics, p) and backward
 *   (dgamma, dbeta, dw [9*Cin*64], db [64]) for a given dp [B,H/5,16,64]; replaces tape.gradient through
 *   conv2d_bn + MaxPooling2D of the first block (layers.py:27-37). */
int seld_k_conv1_gram(const float* x, float* G, int B, int H, int Cin);
int seld_k_conv1_train_gram(const float* x, const float* w, const float* bias, const float* gamma, const float* beta,
                            const float* dp, float* p, float* dw, float* db, float* dgamma, float* dbeta, int B, int H, int Cin);
/* p = max(0, zext * scale[c] + shift[c]) (fused multiply-add), n elements, 64 channels innermost */
int seld_k_bn_relu_ext(const float* zext, const float* scale, const float* shift, float* p, int64_t n);
/* input gradient of the same conv (tape.gradient through Conv2D): dz [B,H,W,64] -> dx [B,H,W,Cin=64] */
int seld_k_conv3x3_dgrad(const float* dz, const float* w, float* dx, int B, int H, int W, int Cin, int Cout);
/* kernel+bias gradient of the same conv: dw HWIO, db [Cout] */
int seld_k_conv3x3_wgrad(const float* x, const float* dz, float* dw, float* db, int B, int H, int W, int Cin, int Cout);
/* first conv block backward in one fused pass: given the forward's pre-BN z [B,H,64,64], the batch mean/invstd and
 * the gradient dp w.r.t. the pooled output, returns d(conv kernel) HWIO, d(conv bias), dgamma, dbeta.  Equals
 * seld_k_bn_relu_pool_bwd followed by seld_k_conv3x3_wgrad without materialising dz. */
int seld_k_conv1_bwd_fused(const float* x, const float* z, const float* dp, const float* mean, const float* invstd,
                           const float* gamma, const float* beta, float* dw, float* db, float* dgamma, float* dbeta,
                           int B, int H, int Cin, int pt, int pf);
/* BatchNormalization(training) + ReLU + MaxPooling2D(pt,pf) given scale/shift per channel:
 * p = maxpool(relu(z*scale+shift)) (layers.py:33-35 + simple_conv_block) */
int seld_k_bn_relu_pool_fwd(const float* z, const float* scale, const float* shift, float* p,
                            int B, int H, int W, int C, int pt, int pf);
/* backward of the same: dp -> dz, dgamma, dbeta given batch mean / invstd / gamma / beta */
int seld_k_bn_relu_pool_bwd(const float* z, const float* dp, const float* mean, const float* invstd,
                            const float* gamma, const float* beta, float* dz, float* dgamma, float* dbeta,
                            int B, int H, int W, int C, int pt, int pf);
/* C[M,N] = act(A[M,K] * op(B) + bias); transb=0: B [K,N]; 1: B [N,K]; act 0 none,1 sigmoid,2 tanh */
int seld_k_gemm(const float* A, const float* Bm, const float* bias, float* C, int M, int N, int K,
                int transb, int act, int accumulate);
/* two products sharing A in one launch: C0 = act(A*op(B0)+bias0), C1 = act(A*op(B1)+bias1) (the forward/backward GRU
 * input projections of modules.py:311-316, the first Conv1D of the two heads of modules.py:326-346) */
int seld_k_gemm_pair_n(const float* A, const float* B0, const float* B1, const float* bias0, const float* bias1,
                       float* C0, float* C1, int M, int N, int K, int transb, int act);
/* one product over a concatenated K axis: C = act(A0*op(B0) + A1*op(B1) + bias) (the gradient w.r.t. an input that
 * feeds two layers); K % 32 == 0 is required and anything else is refused */
int seld_k_gemm_pair_k(const float* A0, const float* A1, const float* B0, const float* B1, const float* bias,
                       float* C, int M, int N, int K, int transb, int act, int accumulate);
/* the same products on the split-bf16 path (three exact bf16 terms per operand, 6 bf16 MFMAs per product, fp32
 * accumulation: fp32-level accuracy at 2.7x the fp32 MFMA rate): mode 0 C0 = act(A0 op(B0) + bias0); mode 1 also
 * C1 = act(A0 op(B1) + bias1); mode 2 C0 = act(A0 op(B0) + A1 op(B1) + bias0).  K % 32 == 0 and N % 128 == 0 are
 * required (anything else is refused: the caller uses seld_k_gemm).  This is what the train / predict entry points
 * run for the GRU input projections and the heads' first Conv1D. */
int seld_k_gemm_sb(const float* A0, const float* A1, const float* B0, const float* B1, const float* bias0,
                   const float* bias1, float* C0, float* C1, int M, int N, int K, int transb, int act, int mode);
/* C[K1,N] = A[M,K1]^T * B[M,N] (weight gradients of Dense / GRU kernels; K1 = 128 with N % 128 == 0 runs on the split-bf16
 * kernel with transposed LDS reads, gemm_tn_sb.hip, unless seld_k_set_option("gemm_tn_split_bf16", 0)); colsum (may be NULL): [N] = sum_m B[m,:]
 * (the matching bias gradient, produced by the same launch) */
int seld_k_gemm_tn(const float* A, const float* Bm, float* C, float* colsum, int M, int K1, int N);

/* The same launchers with every argument the train step passes (tests/test_gemm_family_gpu.py).  Refusals: SELD_ERR_INVALID, nothing written.
 *   seld_k_gemm_ex   the fp32 MFMA GEMM with leading dimensions.  mode 0: C = act(A op(B) + bias) (+C); stat_part (may be NULL): the BatchNorm
 *                    partials [(column / 64) * row blocks + row / 64][sum 64 | sum of squares 64] of the product's epilogue (no bias / act /
 *                    accumulate); addg is always refused here.  mode 1: also C1 = act(A op(B1) + bias1).  mode 2: C = act(A op(B) + A1 op(B1)
 *                    + bias) (+C), K % 32 == 0.  mode 3: mode 0, C1 = a copy of C (same ldc).  mode 4: N = n0 + n1 columns of one product,
 *                    nsplit = n0: C [M][n0] = act0(..), C1 [M][n1] = act1(..), act = act0 | act1 << 4, M0 / M1 (may be NULL) copies; ldb = N.
 *                    act: 0 none, 1 sigmoid, 2 tanh, 3 relu.
 *   seld_k_gemm_sb_ex  the split-bf16 GEMM (K % 32 == 0, N % 128 == 0, lda % 4 == 0): B0 / B1 are split inside, transb 0 [K][N], 1 [N][K], 2 a 3x3
 *                    kernel [9][N][ldb] as the matrix of its input-gradient convolution.  backward (needs transb != 0): the four-product form
 *                    under option "bwd_four_products".  mode / act as above (modes 0..2); accum: C += .  stat_part: partials per 128-row block;
 *                    addg + gate4: C[e] += addg[e] where bit (e & 3) of gate4[e >> 2] is set, e = row * ldc + column (ldc % 4 == 0).
 *                    conv_C > 0: A0 is an NHWC image [M = B H W][conv_C] and K = 9 conv_C (3x3 'same').
 *   seld_k_gemm_tn_ex  C [K1][N] = A[M][K1]^T B[M][N] on the fp32 kernel: S > 0 and shift = +-1 take A's rows shifted inside each S-row sequence
 *                    (zero outside it); colsum with want_bias; max_splits 0 = the default; chunk_rows 32 or 64; *nslab = the splits taken.
 *   seld_k_gemm_tn_sb_ex  1..4 jobs (K1 = 128, N % 128 == 0) of the split-bf16 kernel in one launch: A, lda, shift, Bm, C, colsum are arrays
 *                    of njobs entries (colsum NULL unless want_bias).   seld_k_gemm_tn_sb_tiles: its tile mode, K1 % 128 == 0, slab_cap floats of
 *                    slab space; conv_C > 0: A is an NHWC image and K1 = 9 conv_C (the kernel gradient of a 3x3 'same' convolution).
 *   seld_k_reduce_slabs_ex  which 0: out_w[n_w] (+)= sum_z slab[z * stride + i]; 1: [out_w | out_b] from slabs of n_w + n_b; 2: two stages through
 *                    tmp [seld_k_reduce_slabs_groups(nslab)][n_w].   seld_k_reduce_slabs2_batch: which 1 for njobs consecutive groups of nslab slabs.
 *   seld_k_heads_weff / seld_k_heads_grad  the folded head weights [W1 W2 ; b1 W2 + b2] of both heads ([K + 1][n[0] + n[1]], n[0] + n[1] <= 64) and the
 *                    four gradients of each head from F [K][n[0] + n[1]] and cs; every pointer argument but weff, F, cs is an array of two.
 *   seld_k_weight_prep  the merged pre-pass launch and the three stand-alone ones from the same inputs, into separate targets.
 *   seld_k_mul       out = a * b elementwise, n % 4 == 0. */
int seld_k_gemm_ex(const float* A, int lda, const float* Bm, int ldb, const float* bias, float* C, int ldc, int M, int N, int K, int transb, int act,
                   int accumulate, int mode, const float* A1, const float* B1, const float* bias1, float* C1, float* M0, float* M1, int nsplit,
                   float* stat_part, const float* addg);
int seld_k_gemm_sb_ex(const float* A0, const float* A1, int lda, const float* B0, const float* B1, int ldb, int transb, const float* bias0,
                      const float* bias1, float* C0, float* C1, int ldc, int M, int N, int K, int act, int mode, int accum, int backward,
                      float* stat_part, const float* addg, const unsigned char* gate4, int conv_C, int conv_H, int conv_W);
int seld_k_gemm_tn_ex(const float* A, int lda, const float* Bm, int ldb, float* C, float* colsum, int M, int K1, int N, int S, int shift,
                      int want_bias, int max_splits, int chunk_rows, int* nslab);
int seld_k_gemm_tn_sb_ex(int njobs, const float* const* A, const int* lda, const int* shift, const float* const* Bm, int ldb, float* const* C,
                         float* const* colsum, int M, int N, int S, int want_bias, int* nslab);
int seld_k_gemm_tn_sb_tiles(const float* A, int lda, const float* Bm, int ldb, float* C, int M, int K1, int N, int64_t slab_cap, int conv_C, int conv_H,
                            int conv_W, int* nslab);
int seld_k_reduce_slabs_groups(int nslab);
int seld_k_reduce_slabs_ex(int which, const float* slab, int nslab, int64_t stride, float* out_w, int64_t n_w, float* out_b, int64_t n_b, int accumulate,
                           float* tmp);
int seld_k_reduce_slabs2_batch(const float* slab, int nslab, int64_t stride, int njobs, float* const* out_w, float* const* out_b, int64_t n_w, int64_t n_b);
int seld_k_heads_weff(const float* const* w1, const float* const* b1, const float* const* w2, const float* const* b2, const int* n, int K, int Hd, float* weff);
int seld_k_heads_grad(const float* const* w1, const float* const* b1, const float* const* w2, float* const* dw1, float* const* db1, float* const* dw2,
                      float* const* db2, const int* n, int K, int Hd, const float* F, const float* cs);
int seld_k_weight_prep(int na, const float* const* a_src, const int* a_ldb, const int* a_transb, const int* a_K, const int* a_N,
                       unsigned short* const* a_fused, unsigned short* const* a_alone, int nb, const float* const* b_w, const int* b_flip,
                       unsigned short* const* b_fused, unsigned short* const* b_alone, const float* const* w1, const float* const* b1,
                       const float* const* w2, const float* const* b2, const int* n, int K, int Hd, float* weff_fused, float* weff_alone);
int seld_k_mul(const float* a, const float* b, float* out, int64_t n);

/* xception_block's depthwise 3x3 backward on [B,H,16,64] NHWC (xception.hip; spec/XCEPTION_BLOCK.md: the unit is ReLU -> depthwise 3x3 ->
 * pointwise -> BatchNormalization).  dy: the gradient w.r.t. the depthwise OUTPUT; xin: the unit's input (aff == NULL) or, with aff = [scale 64 |
 * shift 64], the PREVIOUS unit's pre-BN tensor z (the activation is then relu(z scale + shift)); add (may be NULL): a residual gradient added to dx;
 * k [3][3][64] (Keras depthwise_kernel [3,3,64,1]).  Outputs: dx [B,H,16,64] = the gradient w.r.t. the (pre-ReLU) input, dk [3][3][64], and — with
 * bn_mean / bn_invstd [64] (aff required, add NULL) — sums [128] = [sum dx | sum dx xhat], xhat = (z - mean) invstd: the previous
 * BatchNormalization's backward sums.  fused = 1: one pass (dw3x3_w16_bwd_fused + two-stage combine + partial fold: the default of the model path,
 * round 5); fused = 0: the separate passes (dw3x3_bwd_data, dw3x3_bwd_w, xc_reduce). */
int seld_k_xc_dw_bwd(const float* dy, const float* k, const float* xin, const float* add, const float* aff, const float* bn_mean,
                     const float* bn_invstd, float* dx, float* dk, float* sums, int B, int H, int fused);
/* xception_block's other kernels, one family per call (xception.hip), with the launchers and combines of the model path.  All tensors NHWC fp32 with
 * 64 channels; aff (may be NULL) = [scale 64 | shift 64] as above; options "xc_w16" / "xc_xcd_map" of seld_k_set_option apply to the depthwise
 * launches.  NULL required pointers and sizes below 1: SELD_ERR_INVALID; what a launcher refuses: SELD_ERR_UNSUPPORTED; both before any launch.
 *
 * The depthwise 3x3 forward alone: y [B,H,W,64] = DepthwiseConv2D(3, 'same', use_bias=False)(relu(x) or relu(x scale + shift)), k [3][3][64].
 * W = 16 runs the row-per-workgroup kernel unless "xc_w16" is 0; any other W the generic kernel. */
int seld_k_xc_dw_fwd(const float* x, const float* k, const float* aff, float* y, int B, int H, int W);
/* One unit's forward on [B,H,16,64]: dwo = the depthwise output, z = dwo wpw (wpw [64 in][64 out], Keras pointwise_kernel), and, with sums != NULL,
 * sums [128] = [sum z | sum z^2] over the pixels (NULL: the launch without statistics, as in inference).  fused = 1: xc_unit_fwd_kernel + the
 * combine of its per-workgroup partials; fused = 0: the depthwise kernel, the fp32 GEMM and xc_reduce, the "xc_fused_fwd" = 0 route. */
int seld_k_xc_unit_fwd(const float* x, const float* kdw, const float* wpw, const float* aff, float* dwo, float* z, float* sums, int B, int H,
                       int fused);
/* The pointwise half of a unit's backward over npix pixels (any npix >= 1): with dz = scale (gy - c1 - (z - mean) invstd c2), c1c2 = [c1 64 | c2 64],
 * f1 [npix,64] = dz wpw^T (the gradient w.r.t. dwo) and dw [64][64] = dwo^T dz.  mode 1: xc_pw_bwd_kernel + the one-stage slab combine; mode 2: the
 * same kernel + the two-stage combine ("xc_nowait"); mode 0: xc_bn_bwd_dz, the TN product + its combine and the fp32 GEMM ("xc_fused_pw_bwd" = 0). */
int seld_k_xc_pw_bwd(const float* z, const float* gy, const float* dwo, const float* wpw, const float* mean, const float* invstd,
                     const float* scale, const float* c1c2, float* f1, float* dw, int64_t npix, int mode);
/* sums [128] = [sum z | sum z^2] over npix pixels (xc_reduce_kernel + combine) */
int seld_k_xc_bn_stats(const float* z, float* sums, int64_t npix);
/* out = z scale + shift (+ res; res may be NULL) */
int seld_k_xc_bn_apply(const float* z, const float* scale, const float* shift, const float* res, float* out, int64_t npix);
/* Training-mode BatchNormalization's backward given the batch's mean / invstd and scale = gamma invstd: dbeta = sum dy, dgamma = sum dy xhat,
 * c1c2 [128] = [dbeta / npix | dgamma / npix] (written), dz = scale (dy - c1 - xhat c2)  (xc_reduce_kernel, bn_bwd_finalize, xc_bn_bwd_dz) */
int seld_k_xc_bn_bwd(const float* z, const float* dy, const float* mean, const float* invstd, const float* scale, float* dz, float* dgamma,
                     float* dbeta, float* c1c2, int64_t npix);
/* Bidirectional(GRU(128, reset_after=True), merge_mode='mul') recurrence (modules.py:311-316).
 * gx_* [B,S,384] = x*kernel + bias[0]; U_* [128,384]; brec_* = bias[1]; h_* [B,S,128]; out = h_f*h_b.
 * saved_* [B,S,128,4] (per unit: z, r, hh, h*U_h+b) may be NULL. */
int seld_k_gru_fwd(const float* gx_f, const float* gx_b, const float* U_f, const float* U_b,
                   const float* brec_f, const float* brec_b, float* h_f, float* h_b,
                   float* saved_f, float* saved_b, float* out, int B, int S, int units);
/* BPTT of the same: dout [B,S,128] -> dgx_* (input-side pre-activation grads), dgh_* (recurrent-side) */
int seld_k_gru_bwd(const float* dout, const float* h_f, const float* h_b, const float* saved_f,
                   const float* saved_b, const float* U_f, const float* U_b, float* dgx_f, float* dgx_b,
                   float* dgh_f, float* dgh_b, int B, int S, int units);
/* The same recurrence under Keras recurrent_dropout (training; modules.py:312-314), as the training context launches it: rm_* [B,128] hold
 * 0 | 1/(1-rate) per (clip, unit), constant over the sequence; the previous state is multiplied by rm before the recurrent product and before
 * the blend.  h_* is the unmasked output, hm_* [B,S,128] = h * rm the masked state sequence the backward pass reads as h_prev; saved_* as above,
 * required.  Null stream, synchronous.  units != 128: SELD_ERR_UNSUPPORTED before any other check; a NULL pointer, B < 1 or S < 1:
 * SELD_ERR_INVALID, nothing enqueued. */
int seld_k_gru_drop_fwd(const float* gx_f, const float* gx_b, const float* U_f, const float* U_b, const float* brec_f, const float* brec_b,
                        const float* rm_f, const float* rm_b, float* h_f, float* h_b, float* hm_f, float* hm_b, float* saved_f, float* saved_b,
                        int B, int S, int units);
/* BPTT of it ('mul' merge: dh = dout * h_other): the carry is the gradient w.r.t. the masked state times rm */
int seld_k_gru_drop_bwd(const float* dout, const float* h_f, const float* h_b, const float* hm_f, const float* hm_b, const float* saved_f,
                        const float* saved_b, const float* U_f, const float* U_b, const float* rm_f, const float* rm_b, float* dgx_f, float* dgx_b,
                        float* dgh_f, float* dgh_b, int B, int S, int units);
/* BinaryCrossentropy + MSE|MMSE on head outputs (train.py:26-29, losses.py:4-13): losses and the
 * gradients w.r.t. the PRE-activation head outputs (sigmoid / tanh folded in). */
int seld_k_losses(const float* sed, const float* doa, const float* y_sed, const float* y_doa,
                  const seld_loss_cfg* cfg, float* sloss, float* dloss, float* dsed_pre, float* ddoa_pre,
                  int B, int S, int nc);
/* Keras Adam update (train.py:311,34); step is 1-based */
int seld_k_adam(float* theta, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                float beta2, float eps, int64_t step);
/* The rest of loss_adam.hip as the fused models' training step launches it, one launcher per entry point (tests/test_step_tail_gpu.py).  Null
 * stream, synchronous.  SELD_ERR_INVALID before any HIP call for: a NULL required pointer, a size below 1, a float4 operand that is not 16-byte
 * aligned, and what each comment below names.
 * seld_k_losses_strided: seld_m_losses with the launcher's remaining arguments.  ld_sed / ld_doa: row strides in floats of dsed_pre / ddoa_pre
 *   (<= 0: dense, nc / 3 nc; a positive stride below the row length is refused) — the fused heads write both into one [rows][n_sed + n_doa]
 *   buffer.  defer_finalize != 0: sloss (and dloss in MMSE mode) are NOT written; seld_k_losses_finalize writes them from the per-workgroup
 *   partials the first call left in `scratch`, which must be untouched in between.  scratch: seld_m_losses_scratch(B * S) floats, 8-byte
 *   aligned; the MMSE denominator sits behind loss_scratch_floats(rows) = 2 rows + 64 of them.  doa_loss outside SELD_DOA_*: refused. */
int seld_k_losses_strided(const float* sed, const float* doa, const float* y_sed, const float* y_doa, const seld_loss_cfg* cfg, float* sloss,
                          float* dloss, float* dsed_pre, int ld_sed, float* ddoa_pre, int ld_doa, float* scratch, int B, int S, int nc,
                          int defer_finalize);
int seld_k_losses_finalize(const seld_loss_cfg* cfg, float* sloss, float* dloss, float* scratch, int B, int S, int nc);
/* utils.adaptive_clip_grad on ONE variable of Keras shape `shape` (HOST array, rank 1..4) at theta + off / g + off: g is clipped in place per
 * unit, theta is only read.  rank outside 1..4, off < 0, a dimension below 1 or more than INT32_MAX elements: refused. */
int seld_k_agc(const float* theta, float* g, int64_t off, int rank, const int64_t* shape_host);
/* dy *= act'(.) from the stored output y = act(.): act 1 sigmoid, 2 tanh, 3 relu (other values refused); n % 4 == 0 */
int seld_k_act_bwd(const float* y, float* dy, int64_t n, int act);
/* models.seldnet_v1's output coupling: out (and out2 unless NULL) [rows, 3 nc] = tanh(doa1 * [sed | sed | sed]); its backward in place on the
 * losses' gradients (ddoa_pre holds d / d(doa1 sed) on entry; dsed_pre is added to).  ld_sed < nc or ld_doa < 3 nc: refused. */
int seld_k_v1_couple_fwd(const float* sed, const float* doa1, float* out, float* out2, int rows, int nc);
int seld_k_v1_couple_bwd(const float* sed, const float* doa1, float* dsed_pre, int ld_sed, float* ddoa_pre, int ld_doa, int rows, int nc);
/* simple_dense_block with kernel_size > 1: xe [B, S, ks * C] lays the ks frames a 'same' Conv1D tap reads side by side (zero outside the clip);
 * time_fold is its transpose, dx [B, S, C] (+)= the taps in order.  C % 4 == 0. */
int seld_k_time_expand(const float* x, float* xe, int B, int S, int C, int ks);
int seld_k_time_fold(const float* dxe, float* dx, int B, int S, int C, int ks, int accumulate);
/* out[r][f] (+)= in[r][f] * mask[r / S][f]: a per-clip mask over the feature axis (the GRU layers' input dropout).  F % 4 == 0. */
int seld_k_mask_rows(const float* in, const float* mask, float* out, int64_t rows, int S, int F, int accumulate);
/* The fused path's dropout (four elements per thread; seld_dropout is the module operator's kernel): out = in * [u >= rate] / (1 - rate) with
 * the uniforms of oracle/seldnet_oracle.py::philox_uniform(n, seed, layer, step).  in == out allowed.  n % 4 == 0, rate in [0, 1). */
int seld_k_dropout4(const float* in, float* out, int64_t n, float rate, uint64_t seed, unsigned layer, unsigned step);
/* The v2 loss stage alone (trainv2.py:38-44), like seld_k_losses: sed / y_sed [B,S,nc], doa / y_doa [B,S,3nc]; sloss, dloss 1 float each;
 * dsed_pre / ddoa_pre (may be NULL): the objective's gradients w.r.t. the heads' pre-activations.  Refusals as seld_train_fwd_bwd_v2. */
int seld_k_losses_v2(const float* sed, const float* doa, const float* y_sed, const float* y_doa, const seld_v2_cfg* cfg, float* sloss,
                     float* dloss, float* dsed_pre, float* ddoa_pre, int B, int S, int nc);
/* The v2 optimizer stage alone, like seld_k_adam: n_vars variables in flat buffers of n floats, variable i = [rows[i]][cols[i]] at off[i]
 * with one clip unit per column (HOST arrays; offsets ascending, no overlap), reg[i] != 0: regularised.  step is 1-based. */
int seld_k_reg_agc_adabelief(float* theta, float* g, float* m, float* v, int64_t n, int n_vars, const int64_t* off_host,
                             const int32_t* rows_host, const int32_t* cols_host, const int32_t* reg_host, float lr, float beta1, float beta2,
                             float eps, float l2, float clip_factor, int64_t step);
/* Test aid (tests/test_model_gpu.py::test_parity_given_identical_routing): after seld_train_fwd_bwd, the routing decision the
 * backward pass took for every pooled element of conv block `block` — MaxPooling2D's argmax as window position row*pf + col and
 * ReLU's gate (pooled value > 0) — as two device byte arrays [B, H/pt, W/pf, 64].  MaxPoolGrad / ReluGrad of the reference
 * (layers.py:33-37 + simple_conv_block) take the same decisions from their own fp32 values; windows whose two largest elements
 * are within one rounding of each other may decide differently.  Synchronises the ctx stream. */
int seld_debug_pool_routing(seld_ctx* ctx, int block, unsigned char* pos, unsigned char* gate);
/* Test aid for resnet50_block (tests/test_model_gpu.py::test_resnet50_gru_train_step): after seld_train_fwd_bwd, the output of one
 * of bottleneck block `block`'s three ReLUs (which = 0: after the 1x1 reduce, 1: after the 3x3, 2: the block output), copied to the
 * device buffer `dst` (capacity floats); *count = its size, [B, T/5, W_block, w or 4w].  output > 0 is the gate the backward pass
 * used.  Synchronises the ctx stream. */
int seld_debug_relu_output(seld_ctx* ctx, int block, int which, float* dst, int64_t capacity, int64_t* count);
/* Test aids, the inverse of the two above (tests/test_model_gpu.py::test_full_size_parity_given_fp64_decisions): make every LATER backward
 * pass of this ctx take GIVEN decisions at a list of elements — host arrays of n flat indices into the decision tensor ([B, H/pt, W/pf,
 * 64] of conv block `block`; the ReLU output of seld_debug_relu_output(block, which)) and n values (routing: 0 = the window passes 0,
 * 1 + pos = it passes the element at window position pos; gate: 0 | 1).  n = 0 clears the list of that tensor.  MaxPoolGrad / ReluGrad of
 * the reference (layers.py:33-37) take these decisions from their own values; among the ~10^7..10^8 decisions of a full-size step a few
 * dozen (conv blocks) to a few thousand (the 16-bottleneck resnet) sit within fp32 rounding of a tie and decide differently in ANY two
 * evaluations.  With the fp64 oracle's decisions injected at exactly those elements (the fixtures carry them:
 * tests/golden/make_golden_*.py), the step's gradients are comparable with the free-running fp64 oracle's at the parity bar itself.
 * Implementation: the stored tensors the backward kernels read a decision from are edited by the smallest amount that makes them
 * decide as told (an ulp walk on one pre-BN value, the recorded argmax byte, a 1e-35 in place of a 0), after the forward pass has
 * finished with them.  Not for production use; calls synchronise the ctx stream. */
/* xception_block (spec/XCEPTION_BLOCK.md): seld_debug_pool_routing / _set_routing take block = 1 for the EXIT's MaxPool(ReLU(.)) over (1, 8)
 * ([B, T/5, 2, 64]); seld_debug_relu_output / _set_relu_gates take block = unit index 3 b + u, which = 0, for the ReLU in front of that
 * unit's SeparableConv2D ([B, T/5, 16, 64]; the read returns the value whose sign is the gate). */
int seld_debug_set_routing(seld_ctx* ctx, int block, int64_t n, const int64_t* idx_host, const unsigned char* val_host);
int seld_debug_set_relu_gates(seld_ctx* ctx, int block, int which, int64_t n, const int64_t* idx_host, const unsigned char* val_host);
/* ---- module operators (module_ops.hip): what seld_amd/modules.py composes the reference's configurable blocks from — modules.mother_block
 * / mother_stage (modules.py:15-43, 184-298: Conv2D(k, 'same', strides) + BatchNormalization + skip / projection / concatenation +
 * squeeze-and-excitation), and, around them, bidirectional_GRU_block and simple_dense_block at ANY feature width.  NHWC fp32 device tensors,
 * asynchronous on `stream`, no allocation (scratch is the caller's), any channel count / kernel / stride.  The dense products run on the
 * fp32 MFMA GEMM of gemm.hip; everything else is memory-bound elementwise / reduction work.
 * Refusals: every operator returns SELD_ERR_INVALID, before anything is enqueued, for a NULL required pointer (all but gemm's bias, gemm_tn's
 * colsum, the BatchNormalization scratch, scale_hw_bwd_dx's dmean, gru_fwd's saved_* / out and losses' dsed_pre / ddoa_pre), a size < 1 (B, H, W, C, S, HW, npix, rows, n, nc, M, N, K, K1, kernel and stride extents; count of bn_moving), an unknown kind /
 * mode, copy_channels with off < 0 or off + Cs > Cd, gemm_tn with seq < 0 or M % seq != 0; the GRU operators return SELD_ERR_UNSUPPORTED for
 * units != 128.  The *_scratch size functions return -1 for a size < 1.  A call that passes these checks is launched. */
int seld_m_conv_out(int in, int stride);      /* TensorFlow 'SAME': ceil(in / stride); SELD_ERR_INVALID for in < 1 or stride < 1 */
/* col[(b,ho,wo)][(ki,kj,c)] of Conv2D(k, 'same', strides) on x [B,H,W,C]; the convolution is col * kernel[kh kw C, filters] + bias */
int seld_m_im2col(const float* x, float* col, int B, int H, int W, int C, int kh, int kw, int sh, int sw, void* stream);
int seld_m_col2im(const float* dcol, float* dx, int B, int H, int W, int C, int kh, int kw, int sh, int sw, int accumulate, void* stream);
int seld_m_gemm(const float* A, const float* Bm, const float* bias, float* Cm, int M, int N, int K, int transb, int accumulate, void* stream);
int64_t seld_m_gemm_tn_scratch(int K1, int N);
int seld_m_gemm_tn(const float* A, const float* Bm, float* Cm, float* colsum, float* slab, int M, int K1, int N, int seq, int shift, void* stream);
/* tf.keras.layers.BatchNormalization, training mode (layers.py:33, modules.py:232-268): batch mean / biased variance per channel ... */
int64_t seld_m_bn_scratch(int C);   /* floats of caller scratch seld_m_bn_stats / seld_m_bn_bwd take (two-stage sums that fill the card; NULL: one workgroup per channel) */
int seld_m_bn_stats(const float* z, int64_t npix, int C, float* mean, float* var, float* scratch, void* stream);
/* ... out (+)= (z - mean) rsqrt(var + eps) gamma + beta (inference: mean / var = the moving statistics) ... */
int seld_m_bn_apply(const float* z, const float* mean, const float* var, const float* gamma, const float* beta, float eps, float* out,
                    int64_t npix, int C, int accumulate, void* stream);
/* ... moving = moving * momentum + batch * (1 - momentum), the variance Bessel-corrected by count / (count - 1) ... */
int seld_m_bn_moving(const float* mean, const float* var, float* mov_mean, float* mov_var, int C, float momentum, int64_t count, void* stream);
/* ... and its gradient: dgamma, dbeta, dz */
int seld_m_bn_bwd(const float* z, const float* dy, const float* mean, const float* var, const float* gamma, float eps, float* dz, float* dgamma,
                  float* dbeta, int64_t npix, int C, float* scratch, void* stream);
#define SELD_ACT_SWISH 4
/* y = act(x); dx (+)= dy act'(x) from the pre-activation x.  kind: SELD_ACT_NONE / _SIGMOID / _TANH / _RELU / _SWISH */
int seld_m_act(const float* x, float* y, int64_t n, int kind, void* stream);
int seld_m_act_bwd(const float* x, const float* dy, float* dx, int64_t n, int kind, int accumulate, void* stream);
int seld_m_axpy(float* dst, const float* src, int64_t n, float alpha, void* stream);      /* dst += alpha src */
/* tf.keras.layers.Dropout(rate) in training, on the library's counter-based draws: out[e] = (accumulate ? out[e] : 0) + alpha in[e] M[e], M[e] = 0
 * where u[e] < rate, else 1 / (1 - rate); u = the Philox4x32-10 uniforms of (seed, layer, step, e) that the fused path's Dropout draws (word e & 3
 * of counter (e >> 2, layer, step, e >> 34) under the key (seed lo, seed hi), u = (word >> 8) * 2^-24), at any n >= 1.  A pure function of its
 * arguments: the backward calls it again on the gradient, in place (in == out with accumulate 0 is allowed).  x + f Dropout(y) is one call with
 * alpha = f, accumulate = 1.  SELD_ERR_INVALID for a NULL pointer, n < 1 or a rate outside [0, 1).  Under the seld_m_* contract (module_ops.hip), named
 * with seld_attn_drop_*, the other half of the composed path's Dropout; tests/test_dropout_gpu.py calls it. */
int seld_dropout(const float* in, float* out, int64_t n, float rate, float alpha, int accumulate, uint64_t seed, unsigned layer, unsigned step,
                   void* stream);
/* tf.concat(axis=-1) piece: mode 0 dst[r][off + c] = src[r][c]; mode 1 (its gradient) src[r][c] += dst[r][off + c] */
int seld_m_copy_channels(float* src, float* dst, int64_t rows, int Cs, int Cd, int off, int mode, void* stream);
/* squeeze-and-excitation (modules.py:287-294): reduce_mean over (H, W); out = se * out; and their gradients */
int seld_m_mean_hw(const float* x, float* out, int B, int HW, int C, void* stream);
int seld_m_scale_hw(const float* x, const float* s, float* y, int B, int HW, int C, void* stream);
int seld_m_scale_hw_bwd_ds(const float* x, const float* dy, float* ds, int B, int HW, int C, void* stream);
int seld_m_scale_hw_bwd_dx(const float* dy, const float* s, const float* dmean, float* dx, int B, int HW, int C, int accumulate, void* stream);
/* The recurrent block (modules.py:302-319), the losses (train.py:26-34, losses.py:4-13) and Adam (train.py:311) as module operators: the same
 * kernels as seld_k_gru_fwd / _bwd / seld_k_losses / seld_k_adam, enqueued on the caller's stream with no host synchronisation (round 5: a
 * composed train step runs without one).  seld_m_losses takes its scratch from the caller: seld_m_losses_scratch(B * S) floats. */
int seld_m_gru_fwd(const float* gx_f, const float* gx_b, const float* U_f, const float* U_b, const float* brec_f, const float* brec_b, float* h_f,
                   float* h_b, float* saved_f, float* saved_b, float* out, int B, int S, int units, void* stream);
int seld_m_gru_bwd(const float* dout, const float* h_f, const float* h_b, const float* saved_f, const float* saved_b, const float* U_f,
                   const float* U_b, float* dgx_f, float* dgx_b, float* dgh_f, float* dgh_b, int B, int S, int units, void* stream);
/* The reference's configurable recurrent block, modules.RNN_block / RNN_stage (modules.py:64-83, 322-347): rnn_type GRU | LSTM, one direction or
 * Bidirectional with merge_mode mul | concat | ave | sum.  Module operators under the seld_m_* contract above, named seld_rnn_* as the attention
 * operators are named seld_attn_*: the seld_m_* set is the one tests/test_module_ops_gpu.py calls one by one; these have tests/test_rnn_gpu.py.
 * Contract of the four recurrence entries: SELD_ERR_UNSUPPORTED for units != 128 before any
 * other check (and, after the checks below, for S beyond 2^20); SELD_ERR_INVALID, before anything is enqueued, for a NULL required pointer, B or
 * S < 1, and a half-given second direction.  A NULL gx_b (forward) / dh_b (backward) means ONE direction (bidirectional=False: grid B); every
 * other *_b argument must then be NULL too.
 * LSTM(128, return_sequences=True) recurrence (modules.py:337-340; Keras defaults: gate order i | f | c | o, one bias, tanh / sigmoid; lstm.hip):
 * gx_* [B,S,512] = x*kernel + bias; U_* [128,512] = recurrent_kernel; h_*, c_* [B,S,128] (the backward layer writes at the time index it
 * consumed); saved_* [B,S,128,4] (per unit: the activations i, f, g, o).  c_* and saved_* are written for the backward pass only: both NULL
 * (inference) or both given, per call; h is bit-identical either way. */
int seld_rnn_lstm_fwd(const float* gx_f, const float* gx_b, const float* U_f, const float* U_b, float* h_f, float* h_b, float* c_f, float* c_b,
                      float* saved_f, float* saved_b, int B, int S, int units, void* stream);
/* BPTT of the same: dh_* [B,S,128], the gradient w.r.t. each direction's output sequence -> dgx_* [B,S,512], the pre-activation gradients (no
 * reset gate: input side and recurrent side are the same tensor).  dkernel = x^T dgx, dbias = colsum dgx, dU = h_prev^T dgx (seld_m_gemm_tn with
 * seq = S, shift = -1 | +1), dx = dgx kernel^T. */
int seld_rnn_lstm_bwd(const float* dh_f, const float* dh_b, const float* c_f, const float* c_b, const float* saved_f, const float* saved_b,
                      const float* U_f, const float* U_b, float* dgx_f, float* dgx_b, int B, int S, int units, void* stream);
/* GRU(128) per direction (modules.py:334-340): seld_m_gru_fwd without the 'mul' merge, seld_m_gru_bwd with the two directions' output gradients
 * dh_f, dh_b used as given in place of dout * h_other.  The same kernels (gru.hip), other template instantiations. */
int seld_rnn_gru_fwd(const float* gx_f, const float* gx_b, const float* U_f, const float* U_b, const float* brec_f, const float* brec_b, float* h_f,
                     float* h_b, float* saved_f, float* saved_b, int B, int S, int units, void* stream);
int seld_rnn_gru_bwd(const float* dh_f, const float* dh_b, const float* h_f, const float* h_b, const float* saved_f, const float* saved_b,
                     const float* U_f, const float* U_b, float* dgx_f, float* dgx_b, float* dgh_f, float* dgh_b, int B, int S, int units,
                     void* stream);
/* The same GRU recurrence and BPTT at ANY width units = u, 1 <= u <= 256 (gru_w.hip; the architecture search of nas_seldnet draws
 * bidirectional_GRU_stage widths from 4 to 256).  The contract of seld_rnn_gru_fwd / _bwd with 128 read as u: gx_* [B,S,3u] (z | r | h), U_* [u,3u],
 * brec_* [3u], h_* [B,S,u], saved_* [B,S,u,4] = z, r, hh, gh_h (NULL at inference; h has the same bits either way), dh_* [B,S,u] used as given,
 * dgx_* / dgh_* [B,S,3u]; all *_b NULL = one direction.  No alignment beyond 4 bytes is assumed.  Refusals, in this order and before anything is
 * enqueued: SELD_ERR_UNSUPPORTED for units outside 1..256; SELD_ERR_INVALID for a NULL required pointer, B or S < 1, a half-given direction;
 * SELD_ERR_UNSUPPORTED for B or S above 2^30 or B * S above 2^40.  Exact fp32, fixed summation order, a clip's bits do not depend on the batch.
 * seld_rnn_gruw_plan (no device needed): out = {kernel form (0: U in LDS, 1: U re-read through L2 every step), clips per workgroup, forward
 * staging depth in steps, backward staging depth} for that width; returns the number of forms, SELD_ERR_UNSUPPORTED outside 1..256. */
int seld_rnn_gruw_fwd(const float* gx_f, const float* gx_b, const float* U_f, const float* U_b, const float* brec_f, const float* brec_b, float* h_f,
                      float* h_b, float* saved_f, float* saved_b, int B, int S, int units, void* stream);
int seld_rnn_gruw_bwd(const float* dh_f, const float* dh_b, const float* h_f, const float* h_b, const float* saved_f, const float* saved_b,
                      const float* U_f, const float* U_b, float* dgx_f, float* dgx_b, float* dgh_f, float* dgh_b, int B, int S, int units,
                      void* stream);
int seld_rnn_gruw_plan(int units, int32_t out[4]);
/* The same recurrences under Keras dropout / recurrent_dropout (modules.py:312-315, 338-340 pass dropout_rate as both), training only; the
 * contract of the four entries above, with every buffer the backward reads REQUIRED (the masks, c_*, hm_*, saved_*).  rm_* [B,128]: the state
 * mask of each direction, 0 | 1/(1-rate) per (clip, unit), constant over the sequence.  The input mask is not these entries' business: the
 * caller projects x * im (seld_rnn_mask_rows) into gx_*.
 * LSTM (LSTMCell.call, implementation 2): z = gx[t] + (h_prev rm) U; c' = f c + i g, c is never masked; h' = o tanh(c'), emitted unmasked.
 * The kernels scale their register copy of U by rm (lstm.hip), so h_*, c_*, saved_* are laid out as by seld_rnn_lstm_fwd and a mask of ones
 * gives its bits.  BPTT: the carry into the previous step is rm (dgx[t] U^T); dU = (h_prev rm)^T dgx (seld_rnn_mask_rows on h_*, then
 * seld_m_gemm_tn with seq = S, shift = -1 | +1). */
int seld_rnn_lstm_drop_fwd(const float* gx_f, const float* gx_b, const float* U_f, const float* U_b, const float* rm_f, const float* rm_b,
                           float* h_f, float* h_b, float* c_f, float* c_b, float* saved_f, float* saved_b, int B, int S, int units, void* stream);
int seld_rnn_lstm_drop_bwd(const float* dh_f, const float* dh_b, const float* c_f, const float* c_b, const float* saved_f, const float* saved_b,
                           const float* U_f, const float* U_b, const float* rm_f, const float* rm_b, float* dgx_f, float* dgx_b, int B, int S,
                           int units, void* stream);
/* GRU (GRUCell.call, implementation 2, reset_after=True; seld_k_gru_drop_fwd / _bwd per direction and on `stream`): h_prev rm goes into the
 * recurrent product AND the blend; h_* is the unmasked output, hm_* [B,S,128] = h rm the masked state sequence, which the backward reads in
 * h_*'s place (and the caller as the shifted operand of dU); dh_* are the two directions' output gradients, used as given. */
int seld_rnn_gru_drop_fwd(const float* gx_f, const float* gx_b, const float* U_f, const float* U_b, const float* brec_f, const float* brec_b,
                          const float* rm_f, const float* rm_b, float* h_f, float* h_b, float* hm_f, float* hm_b, float* saved_f, float* saved_b,
                          int B, int S, int units, void* stream);
int seld_rnn_gru_drop_bwd(const float* dh_f, const float* dh_b, const float* hm_f, const float* hm_b, const float* saved_f, const float* saved_b,
                          const float* U_f, const float* U_b, const float* rm_f, const float* rm_b, float* dgx_f, float* dgx_b, float* dgh_f,
                          float* dgh_b, int B, int S, int units, void* stream);
/* seld_k_mask_rows on `stream`, asynchronous, with the same refusals: out[r][f] (+)= in[r][f] * mask[r / S][f]; F % 4 == 0, 16-byte aligned.
 * Named with the recurrence entries it serves: the seld_m_* set is the one tests/test_module_ops_gpu.py calls one by one (above). */
int seld_rnn_mask_rows(const float* in, const float* mask, float* out, int64_t rows, int S, int F, int accumulate, void* stream);
/* Bidirectional(merge_mode) (modules.py:341-342) on h_f, h_b [rows, units]: out / dout [rows, units], or [rows, 2 units] for SELD_MERGE_CONCAT (the
 * forward direction first).  Any units >= 1 (float4 where units % 4 == 0 and the pointers are 16-byte aligned); only SELD_MERGE_MUL reads h_* in the
 * backward (they may be NULL otherwise); SELD_ERR_INVALID for an unknown mode. */
#define SELD_MERGE_MUL 0
#define SELD_MERGE_CONCAT 1
#define SELD_MERGE_AVE 2
#define SELD_MERGE_SUM 3
int seld_rnn_merge_fwd(const float* h_f, const float* h_b, float* out, int64_t rows, int units, int mode, void* stream);
int seld_rnn_merge_bwd(const float* dout, const float* h_f, const float* h_b, float* dh_f, float* dh_b, int64_t rows, int units, int mode,
                       void* stream);
int64_t seld_m_losses_scratch(int rows);
int seld_m_losses(const float* sed, const float* doa, const float* y_sed, const float* y_doa, const seld_loss_cfg* cfg, float* sloss, float* dloss,
                  float* dsed_pre, float* ddoa_pre, float* scratch, int B, int S, int nc, void* stream);
int seld_m_adam(float* theta, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps, int64_t step, void* stream);
/* The v2 recipe (trainv2.py:23-56, swa.py) for composed models, as stream operators under the seld_m_* contract: asynchronous on `stream`,
 * no host synchronisation, every argument check before the first HIP call.  They carry the recipe's seld_v2_ prefix, not seld_m_: like the
 * attention, LayerNorm and recurrence operators below they are not part of the mother-block operator set that
 * tests/test_module_ops_gpu.py enumerates by that prefix.
 * seld_v2_losses: seld_k_losses_v2 (same refusals, same bits) on caller scratch of seld_v2_losses_scratch(B * S) floats, 8-byte aligned
 *   (the denominator of the weighted MMSE sits behind the partials); dense gradient rows.
 * seld_v2_plan_create: the device tables of the optimizer stage for n_vars variables in flat buffers of n floats — the arguments and
 *   refusals of seld_k_reg_agc_adabelief (HOST arrays) — built once: the one call of this group that allocates and copies (on the current
 *   device).  *plan is NULL on failure.  seld_v2_plan_destroy frees it (NULL: nothing).
 * seld_v2_opt: regulariser + AGC (clip_factor <= 0: none) + AdaBelief in two launches, the bits of seld_k_reg_agc_adabelief on the same
 *   buffers; g is overwritten with the gradient the optimizer consumed; step is 1-based.
 * seld_v2_swa: swa = (swa cnt + w) / (cnt + 1), each operation rounded to float32 as numpy evaluates swa.py:29-31; cnt == 0 copies. */
int64_t seld_v2_losses_scratch(int rows);
int seld_v2_losses(const float* sed, const float* doa, const float* y_sed, const float* y_doa, const seld_v2_cfg* cfg, float* sloss, float* dloss,
                     float* dsed_pre, float* ddoa_pre, float* scratch, int B, int S, int nc, void* stream);
int seld_v2_plan_create(int64_t n, int n_vars, const int64_t* off_host, const int32_t* rows_host, const int32_t* cols_host,
                          const int32_t* reg_host, void** plan);
void seld_v2_plan_destroy(void* plan);
int seld_v2_opt(void* plan, float* theta, float* g, float* m, float* v, float lr, float beta1, float beta2, float eps, float l2,
                  float clip_factor, int64_t step, void* stream);
int seld_v2_swa(float* swa, const float* w, int64_t n, int cnt, void* stream);
/* ---- attention operators (attention.hip): the shared core of the reference's attention blocks — modules.transformer_encoder_block / _stage
 * (modules.py:106-126, 379-407), and of conformer_encoder_block / attention_block (modules.py:410-635, layers.py:268-287).  fp32 device
 * tensors, asynchronous on `stream`, no allocation.  Not seld_m_*: seld_amd/modules.py composes the transformer and conformer blocks from these and seld_m_*.
 *   seld_attn_fwd   tf.keras.layers.MultiHeadAttention's core (modules.py:392-393; the reference's own MultiHeadAttention, layers.py:268-287):
 *                   O[b,n,h,:] = sum_m softmax_m(scale Q[b,n,h,:] . K[b,m,h,:]) V[b,m,h,:].  Q, K, V: [B*S, H*d] row-major views with row strides
 *                   ldq / ldk / ldv floats (>= H*d: column slices of one fused [B*S, 3*H*d] projection need no copy), head h = columns h*d ..
 *                   h*d+d-1; O [B*S, H*d] contiguous; lse [B, H, S] = the rows' log-sum-exp of the scaled logits, saved for the backward (NULL
 *                   at inference: O is bit-identical).  No [B,H,S,S] tensor is formed: K / V tiles stream through LDS under an online
 *                   softmax, the products run on the exact-fp32 MFMA.  Any S >= 1 (edge tiles are masked inside).
 *   seld_attn_bwd   dQ, dK, dV (row strides lddq / lddk / lddv) from Q, K, V, O, dO [B*S, H*d] and lse: the probabilities are recomputed from
 *                   lse, rowsum(dO * O) is computed inside.  No atomics: one kernel owns dQ per query tile, one owns dK / dV per key tile; two
 *                   runs are bit-identical.  scratch: seld_attn_bwd_scratch(B, S, H, d) floats (B*H*S: linear in the rows).
 *   d (the reference's key_dim) must be a multiple of 8 in 8 .. 64: anything else returns SELD_ERR_UNSUPPORTED (the scratch size -1) before
 *   any other check, as units != 128 does in seld_m_gru_*.  Then SELD_ERR_INVALID, before anything is enqueued, for a NULL pointer (all but
 *   lse of seld_attn_fwd), B, S or H < 1, or a row stride < H*d (the product in 64 bits: an H*d beyond INT_MAX is covered by no stride).  Then
 *   SELD_ERR_UNSUPPORTED (the scratch size -1) for a grid B * H * ceil(S / 64) beyond INT_MAX. */
int seld_attn_fwd(const float* Q, const float* K, const float* V, int ldq, int ldk, int ldv, float* O, float* lse, int B, int S, int H, int d,
                  float scale, void* stream);
int64_t seld_attn_bwd_scratch(int B, int S, int H, int d);
int seld_attn_bwd(const float* Q, const float* K, const float* V, int ldq, int ldk, int ldv, const float* O, const float* dO, const float* lse,
                  float* dQ, float* dK, float* dV, int lddq, int lddk, int lddv, float* scratch, int B, int S, int H, int d, float scale,
                  void* stream);
/*   seld_attn_drop_fwd / _bwd   the same with Dropout(rate) on the softmax probabilities, as tf.keras.layers.MultiHeadAttention(dropout = rate) and
 *                   layers.MultiHeadAttention_ (layers.py:253-257) apply it in training: O[b,n,h,:] = sum_m P[n,m] M[b,h,n,m] V[b,m,h,:] with P the
 *                   full softmax (lse is bit-equal to seld_attn_fwd's) and M[b,h,n,m] = 0 where u < rate, else 1 / (1 - rate); u = (word >> 8) *
 *                   2^-24 of word (m & 3) of Philox4x32-10 at counter (m >> 2, layer, step, (b H + h) S + n) under the key (seed lo, seed hi).
 *                   The backward recomputes M from the same arguments (dV = (P M)^T dO, dS = P (M (dO V^T) - rowsum(dO * O))): no mask, no
 *                   [B,H,S,S] tensor is stored, no atomics, two runs are bit-identical.  scratch: seld_attn_bwd_scratch.  rate 0 launches
 *                   exactly what seld_attn_fwd / _bwd launch: the same bits.  Contract of seld_attn_* in the same order, with SELD_ERR_INVALID
 *                   also for a rate outside [0, 1), and last SELD_ERR_UNSUPPORTED for B * H * S beyond 2^32 (the counter word) at rate > 0. */
int seld_attn_drop_fwd(const float* Q, const float* K, const float* V, int ldq, int ldk, int ldv, float* O, float* lse, int B, int S, int H, int d,
                       float scale, float rate, uint64_t seed, unsigned layer, unsigned step, void* stream);
int seld_attn_drop_bwd(const float* Q, const float* K, const float* V, int ldq, int ldk, int ldv, const float* O, const float* dO, const float* lse,
                       float* dQ, float* dK, float* dV, int lddq, int lddk, int lddv, float* scratch, int B, int S, int H, int d, float scale,
                       float rate, uint64_t seed, unsigned layer, unsigned step, void* stream);
/*   seld_attnw_*    the five entries above for ANY head width d in 1 .. 64 (the reference's search spaces carry key_dim 2, 3, 4, 6, 12: nas_seldnet.py
 *                   59-76), with the same arguments.  Layout as seld_attn_*: head h = columns h*d .. h*d+d-1, row strides >= H*d, O / dO [B*S, H*d]
 *                   contiguous; single dwords move, so nothing beyond 4-byte alignment is assumed of a pointer, a stride or H*d.  A d that is no
 *                   multiple of 8 runs the same three kernels at the padded width dp = 8 ceil(d / 8) with the columns dd >= d read as zeros and never
 *                   written: a zero column adds exact zeros to every product chain, so the values are those of seld_attn_* at dp on zero-padded
 *                   operands with the same `scale` (bit for bit; a zero's sign aside).  A multiple of 8 launches exactly what seld_attn_* launches.
 *                   The dropout mask is a function of (seed, step, layer, b, h, n, m) and does not see d.  As seld_attn_*: no atomics, no [B,H,S,S]
 *                   tensor, two runs are bit-identical, O is bit-identical with and without lse, rate 0 launches what seld_attnw_fwd / _bwd launch.
 *                   scratch: seld_attnw_bwd_scratch(B, S, H, d) floats (B*H*S).
 *   SELD_ERR_UNSUPPORTED (the scratch size -1) for d outside 1 .. 64 before any other check; then the checks of seld_attn_* / seld_attn_drop_* in
 *   their order, B * H * S beyond 2^32 at rate > 0 included.  seld_attn_* themselves keep refusing a d that is no multiple of 8. */
int seld_attnw_fwd(const float* Q, const float* K, const float* V, int ldq, int ldk, int ldv, float* O, float* lse, int B, int S, int H, int d,
                   float scale, void* stream);
int64_t seld_attnw_bwd_scratch(int B, int S, int H, int d);
int seld_attnw_bwd(const float* Q, const float* K, const float* V, int ldq, int ldk, int ldv, const float* O, const float* dO, const float* lse,
                   float* dQ, float* dK, float* dV, int lddq, int lddk, int lddv, float* scratch, int B, int S, int H, int d, float scale,
                   void* stream);
int seld_attnw_drop_fwd(const float* Q, const float* K, const float* V, int ldq, int ldk, int ldv, float* O, float* lse, int B, int S, int H, int d,
                        float scale, float rate, uint64_t seed, unsigned layer, unsigned step, void* stream);
int seld_attnw_drop_bwd(const float* Q, const float* K, const float* V, int ldq, int ldk, int ldv, const float* O, const float* dO, const float* lse,
                        float* dQ, float* dK, float* dV, int lddq, int lddk, int lddv, float* scratch, int B, int S, int H, int d, float scale,
                        float rate, uint64_t seed, unsigned layer, unsigned step, void* stream);
/*   seld_ln_fwd    tf.keras.layers.LayerNormalization over the last axis of [rows, C] (modules.py:395, 403: biased variance, eps inside the
 *                   square root): y = xhat gamma + beta, xhat = (z - mean z) / sqrt(var z + eps), z = x + r — the residual r may be NULL, so
 *                   LayerNormalization()(x + attn) is one pass.  xhat [rows, C] and rstd [rows] are saved for the backward (both may be NULL
 *                   at inference).  Any C >= 1.
 *   seld_ln_bwd     dz (the gradient of the summed input z: the caller routes it to both addends), dgamma, dbeta from dy and the saved xhat /
 *                   rstd.  dgamma / dbeta: a two-stage column reduction through scratch (seld_ln_scratch(rows, C) floats), no atomics.
 *   SELD_ERR_INVALID for a NULL required pointer (all but r, xhat and rstd of seld_ln_fwd), rows < 1 or C < 1; seld_ln_scratch returns -1. */
int seld_ln_fwd(const float* x, const float* r, const float* gamma, const float* beta, float eps, float* y, float* xhat, float* rstd, int64_t rows,
                int C, void* stream);
int64_t seld_ln_scratch(int64_t rows, int C);
int seld_ln_bwd(const float* dy, const float* xhat, const float* rstd, const float* gamma, float* dz, float* dgamma, float* dbeta, float* scratch,
                int64_t rows, int C, void* stream);
/* ---- conformer operators (conformer.hip): what modules.conformer_encoder_block (modules.py:410-508) needs beyond seld_attn_* / seld_ln_* /
 * seld_m_*.  fp32 device tensors, asynchronous on `stream`, no allocation.
 *   seld_dwconv1d_fwd   the convolution module's GLU and depthwise Conv1D(groups = C, kernel_size k, strides 1, 'same') in one kernel
 *                       (modules.py:476-486): u [B*S, 2C] (glu = 1) or [B*S, C] (glu = 0: attention_block's form, modules.py:603-611) with row
 *                       stride ldu; g[b,s,c] = u[b,s,c] sigmoid(u[b,s,C+c]) (glu = 1) or u[b,s,c]; y[b,s,c] = bias[c] + sum_t w[t,c]
 *                       g[b, s - pl + t, c], pl = (k - 1) / 2, zero outside [0, S) (TensorFlow 'same': an even k pads one frame more behind);
 *                       w [k, C] = Keras' depthwise kernel [k, 1, C]; y [B*S, C] contiguous.  g is formed in the loader and never stored; a
 *                       128-frame tile and its halo are staged once per workgroup in LDS, the channel is the lane.
 *   seld_dwconv1d_bwd   du (row stride lddu; glu = 1: dg sigmoid(b) in the first half, dg a sigmoid(b) (1 - sigmoid(b)) in the second),
 *                       dw [k, C], dbias [C] from u, w and dy [B*S, C].  dw / dbias: two stages through scratch
 *                       (seld_dwconv1d_bwd_scratch(B, S, C, k) floats, bounded in the rows), no atomics: two runs are bit-identical.
 *   1 <= k <= 64; any B, S (k > S included), C >= 1.  SELD_ERR_INVALID, before anything is enqueued, for a NULL pointer, a size < 1, k > 64,
 *   glu not 0 / 1, or a row stride below (glu + 1) * C (the product in 64 bits); SELD_ERR_UNSUPPORTED for a grid ceil(C / 64) * ceil(S / 128) * B
 *   beyond INT_MAX.  The scratch query returns -1 for either.
 *   seld_pos_add        x[b, s, :] += enc[s, :] on x [B, S, D]: the positional table of layers.basic_pos_encoding (layers.py:53-67), a host-built
 *                       constant, added in one launch (modules.py:450).
 *   seld_head_permute   mode 0: dst [D, H, dk] = src [H, D, dk] (the head-major kernels of layers.MultiHeadAttention_, layers.py:148-168, as the
 *                       [D, H dk] matrix seld_m_gemm takes); mode 1: the inverse (their gradients back). */
int seld_dwconv1d_fwd(const float* u, int ldu, const float* w, const float* bias, float* y, int B, int S, int C, int k, int glu, void* stream);
int64_t seld_dwconv1d_bwd_scratch(int B, int S, int C, int k);
int seld_dwconv1d_bwd(const float* u, int ldu, const float* w, const float* dy, float* du, int lddu, float* dw, float* dbias, float* scratch, int B,
                      int S, int C, int k, int glu, void* stream);
int seld_pos_add(float* x, const float* enc, int B, int S, int D, void* stream);
int seld_head_permute(const float* src, float* dst, int H, int D, int dk, int mode, void* stream);
/* ---- relative-position attention (relattn.hip): the core of layers.RelPositionMultiHeadAttention (layers.py:332-392), the attention of
 * modules.attention_block with abs_pos_encoding = False (modules.py:585-588), and attention_block's GLU (modules.py:598-601).  fp32 device
 * tensors, asynchronous on `stream`, no allocation.
 *   seld_relattn_fwd    O[b,n,h,:] = sum_m softmax_m(scale (qu[b,n,h,:] . K[b,m,h,:] + shifted[b,h,n,m])) V[b,m,h,:], qu = Q + u, qv = Q + vb
 *                       (layers.py:374-375), shifted = relative_shift(G) of G[b,h,n,m] = qv[b,n,h,:] . P[m,h,:] (layers.py:360-365, 378-379):
 *                       pad one zero column in front, reshape [S, S+1] -> [S+1, S], drop the first row — shifted[i,j] = G[i, S-1-i+j] for
 *                       j <= i, 0 for j = i+1, G[i+1, j-i-2] for j >= i+2 (the NEXT query row: the reference's behaviour).  `scale` multiplies
 *                       the summed logits (layers.py:383-384).  Q, K, V: [B*S, H*d] views with row strides ldq / ldk / ldv, as seld_attn_fwd
 *                       takes them; P [S, H*d] (row stride ldp): the projected positional table, without a batch axis (layers.py:372); u, vb
 *                       [H*d]: pos_bias_u / pos_bias_v; O [B*S, H*d] contiguous; lse [B, H, S] (NULL at inference: O is bit-identical).
 *                       Neither a [B,H,S,S] nor a [B,H,S,S+1] tensor is formed: the positional term of a logit tile is the product of the
 *                       tile's queries with 127 consecutive rows of the table, read back along the skewed diagonal through LDS.
 *   seld_relattn_bwd    dQu, dQv (the gradients of qu and qv: the caller adds them for dQ and column-sums them for the two biases), dK, dV
 *                       (row strides lddqu / lddqv / lddk / lddv) and dP [S, H*d] (row stride lddp), already summed over the batch, from Q, K,
 *                       V, P, u, vb, O, dO [B*S, H*d] and lse.  The backward of relative_shift is the same index map (every G[i,m] is read
 *                       once).  No atomics: every output element is owned by one lane or added in a fixed order through scratch
 *                       (seld_relattn_bwd_scratch(B, S, H, d) = B*H*S*(1 + 2d) floats: linear in the rows); two runs are bit-identical.
 *   d a multiple of 8 in 8 .. 64, else SELD_ERR_UNSUPPORTED (the scratch size -1) before any other check.  Then SELD_ERR_INVALID, before anything
 *   is enqueued, for a NULL pointer (all but lse of seld_relattn_fwd), B, S or H < 1, or a row stride < H*d (the product in 64 bits).  Then
 *   SELD_ERR_UNSUPPORTED (the scratch size -1) for a grid B * H * ceil(S / 64) beyond INT_MAX or S beyond 2^30 - 256.
 *   seld_glu_fwd        y [rows, C] = u[:, :C] * sigmoid(u[:, C:]) of u [rows, 2C] with row stride ldu (modules.py:599-601).
 *   seld_glu_bwd        du (row stride lddu): dy sigmoid(b) in the first half, dy a sigmoid'(b) in the second, sigmoid' formed from
 *                       exp(-|b|) as in seld_dwconv1d_bwd (no cancellation, no overflow).  SELD_ERR_INVALID for a NULL pointer, rows or C < 1
 *                       or a row stride < 2C; SELD_ERR_UNSUPPORTED for rows * C beyond a launch. */
int seld_relattn_fwd(const float* Q, const float* K, const float* V, int ldq, int ldk, int ldv, const float* P, int ldp, const float* u,
                     const float* vb, float* O, float* lse, int B, int S, int H, int d, float scale, void* stream);
int64_t seld_relattn_bwd_scratch(int B, int S, int H, int d);
int seld_relattn_bwd(const float* Q, const float* K, const float* V, int ldq, int ldk, int ldv, const float* P, int ldp, const float* u,
                     const float* vb, const float* O, const float* dO, const float* lse, float* dQu, float* dQv, float* dK, float* dV, float* dP,
                     int lddqu, int lddqv, int lddk, int lddv, int lddp, float* scratch, int B, int S, int H, int d, float scale, void* stream);
int seld_glu_fwd(const float* u, int ldu, float* y, int64_t rows, int C, void* stream);
int seld_glu_bwd(const float* u, int ldu, const float* dy, float* du, int lddu, int64_t rows, int C, void* stream);
/* ---- the front of models.conv_temporal (stem.hip; reference models.py:54-66): conv2d_bn(filters, first_kernel_size, 'same') and
 * MaxPooling2D(first_pool_size, padding).  Under the seld_m_* contract: NHWC fp32, asynchronous on `stream`, no allocation;
 * SELD_ERR_INVALID, before anything is enqueued, for a NULL required pointer or a size < 1.
 *   seld_stem_conv_fwd     z [B,H,W,F] = Conv2D(F, k, strides 1, 'same')(x [B,H,W,Cin]) + bias, kernel [k,k,Cin,F] (Keras).  k odd, 1 .. 7, Cin
 *                          1 .. 16, any F, H, W, B; SELD_ERR_UNSUPPORTED outside that.  No im2col buffer: the halo patch of a 16 x 32 pixel
 *                          tile sits in LDS and the products run on the split-bf16 MFMA (six bf16 products per fp32 product, fp32 sums).
 *   seld_stem_conv_wgrad   dkernel [k,k,Cin,F] = sum over (b,h,w) of x[b,h+dy,w+dx,c] dz[b,h,w,f], dbias [F] = the column sums of dz; exact
 *                          fp32 MFMA.  Two stages in a fixed order, no atomics: two runs give the same bits.  scratch:
 *                          seld_stem_conv_wgrad_scratch(...) floats (a negative error code for arguments the kernel refuses).  There is no
 *                          input gradient: the stem's input is the data.
 *   seld_pool2d_fwd        y [B,Ho,Wo,C] = MaxPooling2D((ph,pw), strides = pool)(x [B,H,W,C]).  same != 0: TensorFlow 'SAME' — Ho = ceil(H / ph),
 *                          pad_total = Ho ph - H, pad_before = pad_total / 2, the surplus behind; padding never wins: a window takes the maximum
 *                          of its in-bounds elements.  same == 0: 'valid', Ho = H / ph (SELD_ERR_INVALID where that is 0).  idx (may be NULL:
 *                          inference, y is bit-identical): the uint8 position i pw + j of the first maximum in row-major window order;
 *                          SELD_ERR_UNSUPPORTED for ph pw > 255.  float4 over the channels where C % 4 == 0 and the pointers are aligned.
 *   seld_pool2d_bwd        dx [B,H,W,C], all of it (no pre-zeroing, no atomics: strides == pool, so an element lies in at most one window):
 *                          dy of its window where the element is the recorded maximum, 0 elsewhere and in the rows / columns 'valid' leaves out. */
int seld_stem_conv_fwd(const float* x, const float* kernel, const float* bias, float* z, int B, int H, int W, int Cin, int k, int F, void* stream);
int64_t seld_stem_conv_wgrad_scratch(int B, int H, int W, int Cin, int k, int F);
int seld_stem_conv_wgrad(const float* x, const float* dz, float* dkernel, float* dbias, float* scratch, int B, int H, int W, int Cin, int k, int F,
                         void* stream);
int seld_pool2d_fwd(const float* x, float* y, unsigned char* idx, int B, int H, int W, int C, int ph, int pw, int same, void* stream);
int seld_pool2d_bwd(const float* dy, const unsigned char* idx, float* dx, int B, int H, int W, int C, int ph, int pw, int same, void* stream);
/* ---- the voice-activity model (vad.hip): models.spectro_temporal_attention_based_VAD (reference models.py:105-163), its loss
 * (models_test.py:59-60) and the irregular frame window (train_vad_baseline.py:76-106), under the seld_m_* contract: fp32 device tensors,
 * asynchronous on `stream`, no allocation, no atomics and fixed summation orders (two runs give the same bits).  SELD_ERR_INVALID, before
 * anything is enqueued, for a NULL required pointer or a size < 1; SELD_ERR_UNSUPPORTED outside a kernel's stated range.
 *   seld_vad_gate_pool_fwd   the spectral tail (models.py:120-122): y [rows, W / 2, C] (contiguous) = max(g[r, 2w, c], g[r, 2w + 1, c]),
 *                            g = a * sigmoid(b) — MaxPooling2D([1, 2]), 'valid': an odd last column is left out.  a, b: [rows, W, C] views whose
 *                            pixels are `ld` >= C floats apart (the two column halves of one [npix, 2 C] product: ld = 2 C).  idx (may be
 *                            NULL: inference, y is bit-identical): one byte per output, 0 | 1 = the column of the pair that won; the first
 *                            maximum stays (v > best, as seld_pool2d_fwd).  Any rows, W >= 2, C >= 1; four channels per thread where
 *                            C % 4 == 0, ld % 4 == 0 and the pointers are aligned.  SELD_ERR_INVALID for W < 2 or ld < C.
 *   seld_vad_gate_pool_bwd   da, db ([rows, W, C] views of pixel stride ld, as a and b), ALL W columns: with s = sigmoid(b) recomputed,
 *                            da = dy s and db = dy a s (1 - s) at the recorded winner, exactly 0 at the loser and in the odd last column.
 *   seld_vad_tattn_fwd       the temporal attention (models.py:145-153) from q [B, Nt] and k, v [B, T, Nt] BEFORE their sigmoid (the
 *                            BatchNormalization outputs).  Column n = d H + h (the head is the fast index of Reshape((Nt / H, H))):
 *                            s[b,t,h] = Nt^-1/2 sum_d sig(q)[b,dH+h] sig(k)[b,t,dH+h];  P = softmax over t of s;  y [B,T,Nt] = sig(v) P[b,t,h];
 *                            score [B,T] = softmax over t of sum_h s.  P [B,T,H] is written for the backward (may be NULL: inference, y and
 *                            score are bit-identical).  One workgroup per clip; every sum over d, t or h runs in an order the shape alone fixes.
 *                            Range: Nt % H == 0, 1 <= H <= Nt <= 512, 1 <= T <= 64 (s lives in LDS: Nt + T H + T floats <= 133,376 B);
 *                            SELD_ERR_UNSUPPORTED beyond, SELD_ERR_INVALID for Nt % H != 0 or H > Nt.
 *   seld_vad_tattn_bwd       dq [B,Nt], dk, dv [B,T,Nt] with respect to the pre-sigmoid inputs from dy [B,T,Nt] and dscore [B,T]; P and score
 *                            as the forward wrote them.  With c = Nt^-1/2: dP[t,h] = sum_d dy sig(v);  dS[t] = score[t] (dscore[t] -
 *                            sum_t' score dscore);  ds[t,h] = P (dP - sum_t' P dP) + dS[t];  dsig(q)[d,h] = c sum_t ds sig(k);  dsig(k) = c ds
 *                            sig(q);  dsig(v) = dy P;  each times sig (1 - sig).  The forward's range.
 *   seld_vad_bce             tf.keras.backend.binary_crossentropy on probabilities, meaned: with pc = clip(p, 1e-7, 1 - 1e-7),
 *                            loss (+)= weight / n sum -(y log(pc + 1e-7) + (1 - y) log(1 - pc + 1e-7));  dp (may be NULL) = weight / n times its
 *                            derivative, 0 where the clip is active.  `accumulate` != 0 adds to *loss (one call per output of the model).
 *                            Two-stage sum in a fixed order; scratch: seld_vad_bce_scratch(n) floats (-1 for n < 1).
 *   seld_vad_windows         seq_to_windows: win [n_windows, Wn, D], win[n,i,:] = x[n + offs[i],:] for x [len, D], n_windows = len - offs[Wn-1].
 *                            offs: HOST array of Wn offsets, non-decreasing, offs[0] = 0 (preprocess_window's result), copied into the
 *                            launch.  SELD_ERR_INVALID for an unsorted table, offs[0] != 0 or len <= offs[Wn-1]; SELD_ERR_UNSUPPORTED for
 *                            Wn > SELD_VAD_MAX_WINDOW.
 *   seld_vad_unwindow        windows_to_seq: seq [n_windows + offs[Wn-1], D], seq[m,:] = sum_i win[m - offs[i], i, :] / (count[m] + 1e-8) over
 *                            the i with 0 <= m - offs[i] < n_windows, added in the order of i. */
#define SELD_VAD_MAX_NT 512
#define SELD_VAD_MAX_T 64
#define SELD_VAD_MAX_WINDOW 64
int seld_vad_gate_pool_fwd(const float* a, const float* b, int ld, float* y, unsigned char* idx, int64_t rows, int W, int C, void* stream);
int seld_vad_gate_pool_bwd(const float* a, const float* b, int ld, const unsigned char* idx, const float* dy, float* da, float* db, int64_t rows,
                           int W, int C, void* stream);
int seld_vad_tattn_fwd(const float* q, const float* k, const float* v, float* y, float* score, float* P, int B, int T, int Nt, int H, void* stream);
int seld_vad_tattn_bwd(const float* q, const float* k, const float* v, const float* P, const float* score, const float* dy, const float* dscore,
                       float* dq, float* dk, float* dv, int B, int T, int Nt, int H, void* stream);
int64_t seld_vad_bce_scratch(int64_t n);
int seld_vad_bce(const float* p, const float* y, float* loss, float* dp, float* scratch, int64_t n, float weight, int accumulate, void* stream);
int seld_vad_windows(const float* x, float* win, const int32_t* offs, int Wn, int64_t len, int D, void* stream);
int seld_vad_unwindow(const float* win, float* seq, const int32_t* offs, int Wn, int64_t n_windows, int D, void* stream);
/* ---- the head of models.vad_architecture (vadarch.hip; reference models.py:98-102): Dense(U, sigmoid) on x [rows, D] (contiguous) with the
 * Keras kernel w [D, U] and bias b [U], U from 1 to SELD_VADARCH_MAX_U, and its backward from seld_vad_bce's loss — exact fp32 FMA chains
 * (no MFMA: a row-dot), x read once.  The seld_m_* contract: fp32 device tensors, asynchronous on `stream`, no allocation, no atomics, fixed
 * summation orders (two runs give the same bits).  SELD_ERR_INVALID, before anything is enqueued, for a NULL required pointer or a size < 1;
 * SELD_ERR_UNSUPPORTED for U > SELD_VADARCH_MAX_U or more rows than one launch covers.
 *   seld_vadarch_head_fwd          p [rows, U] = sigmoid(b[u] + sum_d x[r,d] w[d,u]).  The order of the sum over d depends on D alone (not on
 *                                  rows, the grid or the alignment); float4 loads of x where D % 4 == 0 and x is 16-byte aligned.
 *   seld_vadarch_head_bwd_scratch  floats of `scratch` for (rows, D, U); -1 outside the range.  It never falls as rows grows: scratch sized for
 *                                  the largest batch serves every smaller one.
 *   seld_vadarch_head_bwd          with n = rows U and pc = clip(p, 1e-7, 1 - 1e-7): *loss = weight / n sum -(y log(pc + 1e-7) + (1 - y)
 *                                  log(1 - pc + 1e-7)) (overwritten); dp its derivative, 0 where the clip is active; dz = dp p (1 - p);
 *                                  dx [rows, D] = dz w^T (may be NULL: the head sits on the data; written once, never read),
 *                                  dw [D, U] = x^T dz, db [U] = the column sums of dz.  y [rows, U].  The loss, dw and db are two-stage
 *                                  sums: per chunk of rows (rows alone fixes the chunks), then over the chunks, both in ascending order. */
#define SELD_VADARCH_MAX_U 8
int seld_vadarch_head_fwd(const float* x, const float* w, const float* b, float* p, int64_t rows, int D, int U, void* stream);
int64_t seld_vadarch_head_bwd_scratch(int64_t rows, int D, int U);
int seld_vadarch_head_bwd(const float* x, const float* w, const float* p, const float* y, float* loss, float* dx, float* dw, float* db,
                          float* scratch, int64_t rows, int D, int U, float weight, void* stream);
/* The data path of the voice-activity task (csrc/vad_feat.hip): the front end, frame labels and window batches of
 * vad_dataloader.py and the counters behind the Keras metrics of train_vad_baseline.py.  The seld_m_* contract: fp32 device tensors,
 * asynchronous on `stream`, no allocation after create, no host synchronisation; SELD_ERR_INVALID for NULL or out-of-range scalars before
 * anything is enqueued, SELD_ERR_UNSUPPORTED for sizes with no kernel.  Every device read is bounded by the totals passed as host scalars:
 * a wrong table gives wrong values, never an out-of-range access.  A corpus is PACKED: the utterances lie end to end, file i owns samples
 * sample_starts[i] .. sample_starts[i+1] and rows frame_starts[i] .. frame_starts[i+1] (device int64 [n_files + 1] each).
 *   seld_vad_feat_create     the handle of load_wav_and_extract_feat (vad_dataloader.py:77-98) with get_mel_scale's matrix (109-115): mono,
 *                            hop n_fft / 2; it holds the periodic Hann window, the twiddles and the sparse filter table (each filter a
 *                            contiguous bin range of seld_vad_mel_matrix_host(n_mels, n_fft / 2 + 1, sample_rate, 0, sample_rate / 2)).
 *                            n_fft in {512, 1024, 2048} and 1 <= n_mels <= SELD_VAD_MAX_MELS, SELD_ERR_UNSUPPORTED beyond.
 *                            The tables live on `device`; the caller's current device is the same after the call as before it.  Every
 *                            tensor and the stream given to seld_vad_feat_extract must belong to the handle's device: this is not checked.
 *   seld_vad_feat_frames     host only: frames of tf.signal.stft(frame_length = n_fft, frame_step = n_fft / 2) without padding or centring:
 *                            0 if n_samples < n_fft, else 1 + (n_samples - n_fft) / (n_fft / 2).
 *   seld_vad_mel_matrix_host host only, no device: w [n_bins, n_mels] = tf.signal.linear_to_mel_weight_matrix, built in double and rounded
 *                            once: mel(f) = 1127 ln(1 + f / 700); n_mels + 2 edges equally spaced in mel from lower_hz to upper_hz; bin k at
 *                            k (sample_rate / 2) / (n_bins - 1); weight max(0, min(rising, falling slope)), both slopes in mel; row 0 zero.
 *   seld_vad_feat_extract    out [total_frames, n_mels] (the reference's [frames, n_mels, 1]) from wav [total_samples] (lines 86-97): per
 *                            frame periodic Hann, real FFT (fp32, one frame per transform: a frame's values depend on its samples alone),
 *                            |X| = sqrt(re^2 + im^2), the mel projection in ascending bin order (an empty filter: exactly 0).  logmel:
 *                            log(min(max(s, 1e-8), M)), M the FILE's maximum of s; normalize: (v - min) / (max - min) over the file.  The
 *                            arithmetic is literal: a silent or constant file comes out all NaN, as the reference's does.
 *   seld_vad_frame_labels    load_label (lines 101-106): y [total_frames], y[t] = rintf(sum of labels[s .. s + n_fft) / n_fft) (tf.round: half
 *                            to even) with s the frame's first sample; the sum runs in an order n_fft alone fixes.
 *   seld_vad_gather          apply_window (lines 126-136) for a batch: x_out [B, Wn, D], x_out[b,i,:] = feat[pos[b] + offs[i], :], y_out [B, Wn]
 *                            likewise from y; feat [total_frames, D], pos device int64 [B] (absolute rows), offs the HOST table of
 *                            seld_vad_windows (same refusals), copied into the launch; rows are clamped into [0, total_frames).
 *   seld_vad_score_update    the counters of Keras AUC / Precision / Recall / binary_accuracy (train_vad_baseline.py:49, 216-224): counts
 *                            (device int64 [NT + 1][2], ADDED to) [k][y != 0] += 1 with k the number of thresholds (ascending fp32 device
 *                            table, NT <= 1024) that pred > thr holds for in fp32; a NaN lands in bucket 0.  Integer atomics: exact in any
 *                            order.  The rates, their suffix sums and the trapezoid are the caller's float64 arithmetic. */
#define SELD_VAD_MAX_MELS 256
typedef struct seld_vadfeat seld_vadfeat;
int seld_vad_feat_create(int sample_rate, int n_fft, int n_mels, int device, seld_vadfeat** out);
void seld_vad_feat_destroy(seld_vadfeat* f);
int64_t seld_vad_feat_frames(int n_fft, int64_t n_samples);
int seld_vad_mel_matrix_host(int n_mels, int n_bins, int sample_rate, double lower_hz, double upper_hz, float* w);
int seld_vad_feat_extract(seld_vadfeat* f, const float* wav, const int64_t* sample_starts, const int64_t* frame_starts, int n_files,
                          int64_t total_samples, int64_t total_frames, int logmel, int normalize, float* out, void* stream);
int seld_vad_frame_labels(const float* labels, const int64_t* sample_starts, const int64_t* frame_starts, int n_files, int64_t total_samples,
                          int64_t total_frames, int n_fft, float* y, void* stream);
int seld_vad_gather(const float* feat, const float* y, const int64_t* pos, const int32_t* offs, int Wn, int B, int D, int64_t total_frames,
                    float* x_out, float* y_out, void* stream);
int seld_vad_score_update(const float* pred, const float* y, int64_t n, const float* thresholds, int NT, int64_t* counts, void* stream);
/* Measurement aid (bench.py, SURVEY.md §8(d) "state the step-latency floor"): the shader clock the card holds while `blocks`
 * workgroups of 512 threads run a VALU-only loop (the load shape of the GRU recurrence: 2B workgroups, no MFMA), from
 * s_memtime / s_memrealtime (100 MHz) inside the kernel.  No reference counterpart. */
int seld_k_valu_clock_mhz(int blocks, double* mhz);
/* resnet50_block pieces (spec/RESNET50_BLOCK.md; model_config/resnet50_gru.json:2-11), as the train / predict entry points compose them.
 *   seld_k_rn_conv      z [B,H,W/stride_f,Cout] = Conv2D(Cout, ksize in {1,3}, 'same', strides (1,stride_f), use_bias=False)(x [B,H,W,Cin]);
 *                       w HWIO.  ksize 1: a product on rows of stride Cin*stride_f; ksize 3: a product on im2col rows (formed on load by the
 *                       split-bf16 kernels when Cin and Cout are powers of two >= 128, else materialised); split-bf16 kernels wherever the
 *                       shape allows unless seld_k_set_option("rn_split_bf16", 0), else the fp32 MFMA GEMM.
 *   seld_k_rn_conv_stats  the same, and sums (NULL: not computed): device, ceil(Cout/64)*128 + 1 doubles — per 64-channel chunk
 *                       [sum z | sum z^2] in double from the product's BatchNorm-statistics epilogue (as the training step takes them;
 *                       channels past Cout 0), then M.
 *   seld_k_rn_conv_bwd  dw (HWIO) and dx from dz
 *   seld_k_rn_conv_bwd_add  the same, and addg, gate4 (both NULL, or both given with ksize 1, stride_f 1): dx += addg [gate bit],
 *                       gate4[e >> 2] bit (e & 3), as the training step adds an identity shortcut's gradient (in the product's epilogue
 *                       where it takes it, else behind it).
 *   seld_k_rn_bn        out = [relu](BatchNormalization(training)(z) [+ res]) over npix x C (C % 32 == 0); mean / invstd optional outputs
 *   seld_k_rn_bn_bwd    dz, dgamma, dbeta from dy gated by (mask > 0) (mask may be NULL) */
int seld_k_rn_conv(const float* x, const float* w, float* z, int B, int H, int W, int Cin, int Cout, int ksize, int stride_f);
int seld_k_rn_conv_stats(const float* x, const float* w, float* z, int B, int H, int W, int Cin, int Cout, int ksize, int stride_f, double* sums);
int seld_k_rn_conv_bwd(const float* x, const float* w, const float* dz, float* dw, float* dx, int B, int H, int W, int Cin, int Cout,
                       int ksize, int stride_f);
int seld_k_rn_conv_bwd_add(const float* x, const float* w, const float* dz, float* dw, float* dx, int B, int H, int W, int Cin, int Cout,
                           int ksize, int stride_f, const float* addg, const unsigned char* gate4);
int seld_k_rn_bn(const float* z, const float* gamma, const float* beta, const float* res, float* out, float* mean, float* invstd,
                 int64_t npix, int C, int relu);
int seld_k_rn_bn_bwd(const float* z, const float* dy, const float* mask, const float* gamma, float* dz, float* dgamma, float* dbeta,
                     int64_t npix, int C);
/* hipGetDeviceProperties of `device`: compute units, engine clock (kHz), memory clock (kHz), memory bus width (bits) —
 * bench.py prints the peaks they imply next to the constants its roofline fractions use. */
int seld_device_clocks(int device, int* compute_units, int* clock_khz, int* mem_clock_khz, int* mem_bus_bits);

#ifdef __cplusplus
}
#endif
#endif
