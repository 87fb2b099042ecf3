"""Host-side mirror of the reference's modules.py for the blocks that have no fused kernels of their own: a model is COMPOSED here,
layer by layer, from the module operators of libseld_hip.so (include/seld_hip.h: seld_m_*, plus seld_k_gru_* / seld_k_losses /
seld_k_adam) — the way the reference composes Keras layers (modules.py, models.py:18-32).  Every arithmetic operation is a HIP kernel
behind the C ABI; this file holds shapes, the order of calls and the buffers (torch tensors: device memory and the stream, nothing
else).  There is no CPU or PyTorch fallback.

  mother_block  (reference modules.py:184-298)   Conv2D(k,'same') + BatchNormalization (+ skips: identity / 1x1 Conv2D+BN projection)
                                                  + Activation, three times (strides on the second), concatenation where a layer is
                                                  skipped, squeeze-and-excitation tail; the ValueErrors of modules.py:202-222
  mother_stage  (modules.py:15-43)                `depth` mother_blocks, strides in the first only
  bidirectional_GRU_block (modules.py:302-319), simple_dense_block (modules.py:350-376; Conv1D kernel_size 1): at ANY feature width
  transformer_encoder_block / _stage (modules.py:106-126, 379-407)   MultiHeadAttention(n_head, key_dim)(x, x) + LayerNormalization + two
                                                  Conv1D('same') + LayerNormalization, from seld_attn_* / seld_ln_* (attention.hip) and seld_m_*
  conformer_encoder_block / _stage (modules.py:129-152, 410-508)     half-step FFN, positional table, layers.MultiHeadAttention_, the convolution
                                                  module (pointwise Conv1D, GLU + depthwise Conv1D: seld_dwconv1d_* of conformer.hip,
                                                  BatchNormalization, swish, pointwise Conv1D), half-step FFN, LayerNormalization

  attention_block / _stage (modules.py:155-180, 511-635)             FF modules of Conv1D('same'), MultiHeadAttention_ or (abs_pos_encoding False)
                                                  layers.RelPositionMultiHeadAttention (seld_relattn_* of relattn.hip), GLU (seld_glu_*), the
                                                  depthwise Conv1D module, LayerNormalization in front or behind

  RNN_block / RNN_stage (modules.py:64-83, 322-347)                  GRU or LSTM (units 128: the recurrence kernels of gru.hip / lstm.hip), one direction or
                                                  Bidirectional with merge_mode mul | concat | ave | sum (seld_rnn_*); dropout_rate = Keras dropout and
                                                  recurrent_dropout: per-clip input and state masks in training (seld_rnn_mask_rows, seld_rnn_*_drop_*)

  models.conv_temporal (models.py:54-78)                              ConvTemporalNet: StemConv2D (seld_stem_conv_* of stem.hip) + BatchNormalization + relu +
                                                  MaxPool2D (seld_pool2d_*), the BLOCK* chain (mother blocks, then every 3-D kind, DenseBlock =
                                                  simple_dense_block as a body block) and a block or stage as each head (_StageHead)

  models.vad_architecture (models.py:81-102)                          VadArchNet: the optional flatten, the same BLOCK* chain (DenseBlock with its Dropout layers wired, Dense
                                                  variables on the 2-D tensor) and Dense(last_unit, sigmoid) + binary cross-entropy as one fused head
                                                  (seld_vadarch_head_* of vadarch.hip) or composed from Linear, seld_m_act and seld_vad_bce

The shared pieces, each in one place:
  Linear               GEMM + bias with its backward: Dense, Conv1D and Conv2D (im2col in front of it where the window is wider than one
                       sample), the heads' layers (Head) and the squeeze-and-excitation pair (_SqueezeExcite)
  _FeedForward         layer -> activation -> layer over Dense or Conv1D: the transformer's, both of the conformer's, the attention block's
  _ConvTail            depthwise Conv1D -> BatchNormalization -> swish -> pointwise Conv1D: the conformer's and the attention block's
  _Attention           the attention layers' buffers; _HeadMajorAttention: the reference's own two layers' packing and projections
  _Recurrent           the recurrent blocks' variables, input projections and weight gradients (RNNBlock, BidirectionalGRUBlock)
  _Drop                one block's Dropout layers (transformer, conformer and absolute-position attention blocks, and the recurrent blocks'
                       cell masks; training only): the draw streams and the calls of seld_dropout; the attention probabilities are dropped inside
                       seld_attn_drop_fwd / _bwd
  Stage, SECOND_KINDS  every SECOND kind is a Stage of blocks of one class; the table names the class, its config check and its prefix, and
                       the eight factories and ComposedSeldNet build from it (_second_factory, _build_second)

`ComposedSeldNet` = models.seldnet(input_shape, model_config) for FIRST in {mother_block, mother_stage}, SECOND in {bidirectional_GRU_block,
transformer_encoder_block, transformer_encoder_stage, conformer_encoder_block, conformer_encoder_stage, attention_block, attention_stage, RNN_block,
RNN_stage}: same surface as
seld_amd.models.SeldNet (variables in Keras creation order, get / set_weights, __call__, train.trainstep / teststep).  The three
BASELINE configurations do NOT run through here — their blocks are fused kernels inside a seld_ctx (models.SeldNet)."""
from __future__ import annotations

import copy
import ctypes as C
import math
from typing import Dict, List, Tuple

import numpy as np
import torch

from . import _lib

ACT = {None: 0, "linear": 0, "sigmoid": 1, "tanh": 2, "relu": 3, "swish": 4}
BN_EPS, BN_MOMENTUM = 1e-3, 0.99
LN_EPS = 1e-3      # tf.keras.layers.LayerNormalization's default epsilon


def safe_tuple(v, n=2):
    return tuple(int(a) for a in v) if isinstance(v, (list, tuple)) else (int(v),) * n


def _check_activation(cfg: dict, default: str, key: str = "activation") -> None:
    if cfg.get(key, default) not in ACT:
        raise ValueError(f"{key} {cfg.get(key)!r}: the module operators know {sorted(k for k in ACT if k)}")


DROPOUT_DEFAULT = 0.1      # the reference's default of the three attention kinds (modules.py:386, 416, 529)
DROP_STREAM0 = 4096        # the composed path's first draw stream: clear of the fused path's 16 hd + j, 64 + i and 96 + 4 i + d


def _check_no_dropout(cfg: dict, who: str) -> None:
    if "dropout_rate" not in cfg or float(cfg["dropout_rate"]) != 0.0:
        raise ValueError(f"{who}: the reference's Dropout draws from TensorFlow's generator, which this path cannot reproduce, and the reference's "
                         "default dropout_rate is 0.1: dropout_rate must be present and 0 — or the caller accepts the library's own counter-based "
                         "draws: dropout=True (models.seldnet does)")


def _dropout_rate(cfg: dict, who: str, dropout: bool = True) -> float:
    """dropout_rate as the fp32 the kernels compare with (absent: the reference's 0.1); 0 <= rate < 1.  Without `dropout` (the caller has not
    accepted the library's draws in place of TensorFlow's) the key must be present and 0, as before there were dropout kernels."""
    if not dropout:
        _check_no_dropout(cfg, who)
        return 0.0
    r = cfg.get("dropout_rate", DROPOUT_DEFAULT)
    r = float(np.float32(DROPOUT_DEFAULT if r is None else r))
    if not 0.0 <= r < 1.0:
        raise ValueError(f"{who}: dropout_rate {cfg.get('dropout_rate')!r}: 0 <= dropout_rate < 1")
    return r


def _check_key_dim(key_dim, any_key_dim: bool = False) -> None:
    """any_key_dim: any integer in 1..64 (seld_attnw_*); without it a multiple of 8 from 8 to 64 (seld_attn_*)"""
    if any_key_dim:
        if isinstance(key_dim, (bool, np.bool_)) or not isinstance(key_dim, (int, np.integer)) or not 1 <= int(key_dim) <= 64:
            raise ValueError(f"key_dim {key_dim!r}: with any_key_dim the attention kernels take an integer from 1 to 64")
        return
    dk = int(key_dim)
    if dk < 8 or dk > 64 or dk % 8:
        raise ValueError(f"key_dim {dk}: the attention kernels take a multiple of 8 from 8 to 64")


def _check_pos_encoding(cfg: dict, who: str, D, relative: bool = False) -> None:
    """relative: the table feeds RelPositionMultiHeadAttention, which cannot do without one (reference modules.py:549-551)"""
    pe = cfg.get("pos_encoding", "basic")
    if pe == "rff":
        raise ValueError(f"{who}: pos_encoding 'rff' draws its frequencies from tf.random.normal and stores them nowhere: it cannot be reproduced")
    if pe not in ("basic", None):
        raise ValueError(f"{who}: pos_encoding {pe!r}: 'basic' or None")
    if relative and pe is None:
        raise ValueError("relative pos encoding demands any types of encoding except the null one")
    if pe == "basic" and D is not None and int(D) % 2:
        raise ValueError(f"{who}: pos_encoding 'basic' on an odd width {D}: the reference's table has 2 * (D // 2) columns and does not broadcast")


def check_mother_config(cfg: dict) -> None:
    """reference modules.py:202-222"""
    f = [cfg[f"filters{i}"] for i in range(3)]
    k = [cfg[f"kernel_size{i}"] for i in range(3)]
    c0, c1, c2 = cfg["connect0"], cfg["connect1"], cfg["connect2"]
    strides = safe_tuple(cfg.get("strides", (1, 1)))
    for i in range(3):
        if (f[i] == 0) != (k[i] == 0):
            raise ValueError(f"{i}) skipped layer must have 0 filters, 0 kernel size")
    if f[0] == 0 and max(c1[1], c2[1]):
        raise ValueError("cannot link skipped layer (first layer)")
    if f[1] == 0 and c2[2] > 0:
        raise ValueError("cannot link skipped layer (second layer)")
    if (f[0] != 0) + sum(c0) == 0:
        raise ValueError("cannot pass zero inputs to the second layer")
    if (f[1] != 0) + sum(c1) == 0:
        raise ValueError("cannot pass zero inputs to the third layer")
    if (f[2] != 0) + sum(c2) == 0:
        raise ValueError("cannot pass zero inputs to the final output")
    if f[1] == 0 and tuple(strides) != (1, 1):
        raise ValueError("if strides are set, the second layer must be active")
    for key in ("activation", "se_activation"):
        _check_activation(cfg, "relu", key)


def dead_layers(cfg: dict):
    """(first layer dead, second layer dead): a layer whose output reaches neither the block's output nor a later layer — configurations the
    reference accepts (modules.py:202-222) and whose Keras functional model simply does not contain the layer: no variables, no computation"""
    f = [int(cfg[f"filters{i}"]) for i in range(3)]
    c1, c2 = cfg["connect1"], cfg["connect2"]
    need2 = f[2] > 0 or c2[2] == 1
    need1 = c2[1] == 1 or (need2 and (f[1] > 0 or c1[1] == 1))
    return (f[0] > 0 and not need1), (not need2)


class _Rt:
    """What every layer shares: the library, the device, the variable store and the operator calls (all on torch's current stream)."""

    def __init__(self, device):
        self.lib = _lib.load()
        self.dev = device
        self.tr: List[Tuple[str, Tuple[int, ...]]] = []
        self.nt: List[Tuple[str, Tuple[int, ...]]] = []
        self._views: Dict[str, torch.Tensor] = {}
        self.linears: List[Tuple[int, int, int]] = []      # (rows, K, N) of every Linear built on this runtime: the plan's dense products
        self.recurrent: List[Tuple[int, int, int, int]] = []      # (rows, D, units, G) of every recurrent layer's direction (_Recurrent)
        self.params = self.grads = self.state = None
        self._slab = None
        self._bn_scratch = None
        # Dropout draws, with the semantics of the fused path's context (csrc/ctx.h): every training forward of a model takes
        # dropout_cur = dropout_step++ and its backward recomputes the masks of dropout_cur
        self.dropout_seed = 0x5e1d5e1d5e1d5e1d
        self.dropout_step = 0
        self.dropout_cur = 0
        self.dropout = False      # the blocks built on this runtime may draw (the owner accepted the library's draws: _dropout_rate)
        self.any_units = False    # the GRU blocks built on this runtime may have any width in 1..256 (seld_rnn_gruw_*: ConvTemporalNet search=True)
        self.any_key_dim = False  # the transformer / conformer blocks built on it may have any key_dim in 1..64 (seld_attnw_*: likewise)

    def next_draws(self):
        """a model's training forward begins: new masks (Keras), backward or not"""
        self.dropout_cur = int(self.dropout_step) & 0xffffffff
        self.dropout_step = (self.dropout_cur + 1) & 0xffffffff

    # ---- variables
    def var(self, name, shape, trainable=True):
        (self.tr if trainable else self.nt).append((name, tuple(int(s) for s in shape)))

    def finalize(self):
        n = sum(int(np.prod(s)) for _, s in self.tr)
        ns = sum(int(np.prod(s)) for _, s in self.nt)
        z = lambda k: torch.zeros(max(k, 1), dtype=torch.float32, device=self.dev)
        self.params, self.grads, self.adam_m, self.adam_v, self.state = z(n), z(n), z(n), z(n), z(ns)
        off = 0
        self.variables, self.state_variables = [], []
        for name, sh in self.tr:
            k = int(np.prod(sh))
            self.variables.append((name, off, sh))
            self._views[name] = self.params[off:off + k]
            self._views["d:" + name] = self.grads[off:off + k]
            off += k
        off = 0
        for name, sh in self.nt:
            k = int(np.prod(sh))
            self.state_variables.append((name, off, sh))
            self._views[name] = self.state[off:off + k]
            off += k
        self.n_params, self.n_state = n, ns

    def w(self, name):
        return self._views[name]

    def g(self, name):
        return self._views["d:" + name]

    def empty(self, *shape):
        return torch.empty(shape, dtype=torch.float32, device=self.dev)

    def bn_scratch(self, C):
        """the BatchNormalization sums' first-stage partials: one buffer per channel count, shared by every layer (calls are in stream order)"""
        need = int(self.lib.seld_m_bn_scratch(int(C)))
        if self._bn_scratch is None or self._bn_scratch.numel() < need:
            self._bn_scratch = self.empty(need)        # (torch allocations are 256-byte aligned: the kernels read it as doubles)
        return self._bn_scratch

    # ---- operator calls
    def st(self):
        return C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    @staticmethod
    def p(t):
        return C.c_void_p(t.data_ptr()) if t is not None else None

    def ck(self, rc):
        _lib.check(rc)

    def gemm(self, A, Bm, bias, Cm, M, N, K, transb=0, accumulate=0):
        self.ck(self.lib.seld_m_gemm(self.p(A), self.p(Bm), self.p(bias), self.p(Cm), M, N, K, transb, accumulate, self.st()))

    def gemm_tn(self, A, Bm, Cm, colsum, M, K1, N, seq=0, shift=0):
        need = int(self.lib.seld_m_gemm_tn_scratch(K1, N))
        if self._slab is None or self._slab.numel() < need:
            self._slab = self.empty(need)
        self.ck(self.lib.seld_m_gemm_tn(self.p(A), self.p(Bm), self.p(Cm), self.p(colsum), self.p(self._slab), M, K1, N, seq, shift, self.st()))

    def act(self, x, y, kind):
        self.ck(self.lib.seld_m_act(self.p(x), self.p(y), x.numel(), kind, self.st()))

    def act_bwd(self, x, dy, dx, kind, accumulate=0):
        self.ck(self.lib.seld_m_act_bwd(self.p(x), self.p(dy), self.p(dx), x.numel(), kind, accumulate, self.st()))

    def axpy(self, dst, src, alpha=1.0):
        self.ck(self.lib.seld_m_axpy(self.p(dst), self.p(src), dst.numel(), alpha, self.st()))


class _Drop:
    """One block's Dropout layers (reference modules.py:392-402, 440-502, 566-628): the rate, whether the current forward draws (`on`:
    training and rate > 0 — otherwise every caller launches exactly what it launches without dropout) and the block's draw streams

        layer = DROP_STREAM0 (4096) + 32 * (index of the block in its Stage) + site,      site = the Dropout's rank in reference order:

        site  transformer_encoder_block     conformer_encoder_block          attention_block
        0     attention probabilities       first FFN, behind the activation first FF, behind the activation
        1     behind the attention          first FFN, behind its output     first FF, behind its output
        2     FFN, behind the activation    attention probabilities          attention probabilities
        3     FFN, behind its output        behind the attention             behind the attention
        4                                   behind the convolution module    behind the depthwise tail
        5                                   second FFN, behind the activation second FF, behind the activation
        6                                   second FFN, behind its output    second FF, behind its output

    (a site keeps its number where a configuration leaves its module out); the recurrent blocks (_Recurrent) draw their cells' masks on sites
    0 / 1 = the forward direction's input / state mask, 2 / 3 = the backward direction's.  Element e of a [rows, C] tensor draws word e & 3 of counter
    (e >> 2, layer, step, e >> 34): seld_dropout; the attention probabilities draw inside the kernels: seld_attn_drop_fwd / _bwd.  Nothing is
    stored: the backward calls the same operators with the runtime's dropout_cur.  The rate is above 0 only where the owner of the runtime accepted
    these draws in place of TensorFlow's (_Rt.dropout: a ComposedSeldNet, or a factory called with dropout=True)."""

    def __init__(self, rt: "_Rt", rate: float):
        self.rt, self.rate, self.base, self.on = rt, float(rate), DROP_STREAM0, False

    def begin(self, training) -> None:
        self.on = bool(training) and self.rate > 0.0

    def apply(self, site: int, src, dst, alpha: float = 1.0, accumulate: int = 0):
        """dst (+)= alpha * Dropout(src) with the mask of `site` (forward: activations; backward: gradients); src is dst: in place"""
        rt = self.rt
        rt.ck(rt.lib.seld_dropout(rt.p(src), rt.p(dst), src.numel(), self.rate, alpha, int(accumulate), rt.dropout_seed, self.base + site,
                                    rt.dropout_cur, rt.st()))
        return dst

    def add(self, site: int, dst, src, alpha: float = 1.0) -> None:
        """dst += alpha * Dropout(src): one pass; without dropout the axpy it replaces"""
        if self.on:
            self.apply(site, src, dst, alpha, 1)
        else:
            self.rt.axpy(dst, src, alpha)



class Linear:
    """A layer that is exactly GEMM + bias on [rows, K]: variables `kernel` (of `kshape`, any shape whose product is K * N; default
    [K, N]) and `bias` [N], the output buffer `z`.  backward: kernel / bias gradients by seld_m_gemm_tn; dx (+)= dz kernel^T (dx None: not
    needed).  The buffers hold the LARGEST batch's rows; a call works on its own `rows` only."""

    def __init__(self, rt: _Rt, name: str, rows: int, K: int, N: int, kshape=None):
        self.rt, self.name, self.K, self.N = rt, name, int(K), int(N)
        rt.var(f"{name}.kernel", kshape or (self.K, self.N))
        rt.var(f"{name}.bias", (self.N,))
        self.z = rt.empty(rows, self.N)
        rt.linears.append((int(rows), self.K, self.N))

    def forward(self, x, rows):
        rt = self.rt
        self.a = x
        rt.gemm(x, rt.w(f"{self.name}.kernel"), rt.w(f"{self.name}.bias"), self.z, rows, self.N, self.K)
        return self.z[:rows]

    def backward(self, dz, dx, rows, accumulate=0):
        rt = self.rt
        rt.gemm_tn(self.a, dz, rt.g(f"{self.name}.kernel"), rt.g(f"{self.name}.bias"), rows, self.K, self.N)
        if dx is not None:
            rt.gemm(dz, rt.w(f"{self.name}.kernel"), None, dx, rows, self.K, self.N, transb=1, accumulate=int(accumulate))


class Dense(Linear):
    """tf.keras.layers.Dense(units) on the last axis of [rows, Cin]: Dense(rt, name, rows, Cin, units); kernel [Cin, units]."""


class Conv2D(Linear):
    """tf.keras.layers.Conv2D(filters, k, strides, padding='same', use_bias=True): im2col (skipped for 1x1 stride 1) + the MFMA GEMM over
    the K = k k Cin columns."""

    def __init__(self, rt: _Rt, name: str, in_shape, filters: int, k: int, strides=(1, 1), B: int = 1):
        self.k, self.s = int(k), tuple(strides)
        self.H, self.W, self.Cin = in_shape
        self.Ho, self.Wo = -(-self.H // self.s[0]), -(-self.W // self.s[1])
        super().__init__(rt, name, B * self.Ho * self.Wo, self.k * self.k * self.Cin, filters, (self.k, self.k, self.Cin, int(filters)))
        self.out_shape = (self.Ho, self.Wo, self.N)
        self.direct = self.k == 1 and self.s == (1, 1)
        self.B = B
        self.col = None if self.direct else rt.empty(B * self.Ho * self.Wo, self.K)
        self.dcol = None if self.direct else rt.empty(B * self.Ho * self.Wo, self.K)

    def forward(self, x, B):
        rt = self.rt
        if not self.direct:
            rt.ck(rt.lib.seld_m_im2col(rt.p(x), rt.p(self.col), B, self.H, self.W, self.Cin, self.k, self.k, self.s[0], self.s[1], rt.st()))
            x = self.col
        return Linear.forward(self, x, B * self.Ho * self.Wo).view(B, *self.out_shape)

    def backward(self, dz, dx, B, accumulate):
        """dz [B,Ho,Wo,N] -> kernel / bias gradients; dx (+)= the input gradient (dx None: not needed)"""
        rt = self.rt
        M = B * self.Ho * self.Wo
        if self.direct or dx is None:
            return Linear.backward(self, dz, dx, M, accumulate)
        Linear.backward(self, dz, self.dcol, M)
        rt.ck(rt.lib.seld_m_col2im(rt.p(self.dcol), rt.p(dx), B, self.H, self.W, self.Cin, self.k, self.k, self.s[0], self.s[1],
                                   int(accumulate), rt.st()))


class StemConv2D(Linear):
    """models.conv_temporal's first layer (reference models.py:62: Conv2D(filters, first_kernel_size, 'same') on the input channels): variables
    `kernel` (k, k, Cin, F) and `bias`, the output buffer `z`, as Conv2D has them.  Inside the stem kernels' contract (k odd, 1 .. 7, Cin <= 16)
    the forward is seld_stem_conv_fwd (no im2col buffer) and the kernel / bias gradients are seld_stem_conv_wgrad; outside it (an even k, more
    channels) both are what Conv2D does: seld_m_im2col + the GEMMs.  DIRECT names the passes that run on the stem kernels where the contract
    allows (tools/bench_conv_temporal.py measured both against im2col: DESIGN.md section 3o).  There is no input gradient: the input is the data."""
    DIRECT = {"fwd": True, "wgrad": True}

    def __init__(self, rt: _Rt, name: str, in_shape, filters: int, k: int, B: int = 1, direct=None):
        self.k = int(k)
        self.H, self.W, self.Cin = (int(v) for v in in_shape)
        if self.k < 1 or int(filters) < 1:
            raise ValueError(f"StemConv2D: filters {filters!r} and kernel size {k!r} must be >= 1")
        super().__init__(rt, name, B * self.H * self.W, self.k * self.k * self.Cin, filters, (self.k, self.k, self.Cin, int(filters)))
        self.out_shape = (self.H, self.W, self.N)
        inside = self.k % 2 == 1 and self.k <= 7 and self.Cin <= 16
        direct = dict(self.DIRECT, **(direct or {}))
        self.direct_fwd, self.direct_wgrad = inside and bool(direct["fwd"]), inside and bool(direct["wgrad"])
        self.col = None if (self.direct_fwd and self.direct_wgrad) or self.k == 1 else rt.empty(B * self.H * self.W, self.K)
        self.scratch = rt.empty(int(rt.lib.seld_stem_conv_wgrad_scratch(B, self.H, self.W, self.Cin, self.k, self.N))) if self.direct_wgrad else None

    def _im2col(self, x, B):
        rt = self.rt
        if self.k == 1:
            return x
        rt.ck(rt.lib.seld_m_im2col(rt.p(x), rt.p(self.col), B, self.H, self.W, self.Cin, self.k, self.k, 1, 1, rt.st()))
        return self.col

    def forward(self, x, B):
        rt, n = self.rt, self.name
        self.x = x
        if self.direct_fwd:
            rt.ck(rt.lib.seld_stem_conv_fwd(rt.p(x), rt.p(rt.w(f"{n}.kernel")), rt.p(rt.w(f"{n}.bias")), rt.p(self.z), B, self.H, self.W, self.Cin,
                                            self.k, self.N, rt.st()))
            return self.z[:B * self.H * self.W].view(B, *self.out_shape)
        return Linear.forward(self, self._im2col(x, B), B * self.H * self.W).view(B, *self.out_shape)

    def backward(self, dz, B):
        """dz [B,H,W,F] -> the kernel's and the bias's gradients"""
        rt, n = self.rt, self.name
        if self.direct_wgrad:
            rt.ck(rt.lib.seld_stem_conv_wgrad(rt.p(self.x), rt.p(dz), rt.p(rt.g(f"{n}.kernel")), rt.p(rt.g(f"{n}.bias")), rt.p(self.scratch), B, self.H,
                                              self.W, self.Cin, self.k, self.N, rt.st()))
            return
        if self.direct_fwd:
            self.a = self._im2col(self.x, B)      # the forward did not form the columns
        Linear.backward(self, dz, None, B * self.H * self.W)


class MaxPool2D:
    """tf.keras.layers.MaxPooling2D(pool, strides = pool, padding 'same' | 'valid') on [B, H, W, C]: seld_pool2d_fwd / _bwd.  Owns the
    positions `idx` of the maxima (written in training only), the output and the input gradient."""

    def __init__(self, rt: _Rt, in_shape, pool, B: int, padding: str = "same"):
        self.rt = rt
        self.H, self.W, self.C = (int(v) for v in in_shape)
        self.ph, self.pw = safe_tuple(pool)
        if padding not in ("same", "valid"):
            raise ValueError(f"MaxPool2D: padding {padding!r}: 'same' or 'valid'")
        self.same = int(padding == "same")
        if self.ph < 1 or self.pw < 1 or self.ph * self.pw > 255:
            raise ValueError(f"MaxPool2D: pool {pool!r}: sizes >= 1 whose product is at most 255 (the maximum's position is a uint8)")
        Ho, Wo = (-(-self.H // self.ph), -(-self.W // self.pw)) if self.same else (self.H // self.ph, self.W // self.pw)
        if Ho < 1 or Wo < 1:
            raise ValueError(f"MaxPool2D: pool {pool!r} with padding 'valid' leaves nothing of {tuple(in_shape)}")
        self.out_shape = (Ho, Wo, self.C)
        self.y = rt.empty(B, *self.out_shape)
        self.idx = torch.empty((B,) + self.out_shape, dtype=torch.uint8, device=rt.dev)
        self.dx = rt.empty(B, self.H, self.W, self.C)

    def forward(self, x, B, training):
        rt = self.rt
        rt.ck(rt.lib.seld_pool2d_fwd(rt.p(x), rt.p(self.y), rt.p(self.idx) if training else None, B, self.H, self.W, self.C, self.ph, self.pw,
                                     self.same, rt.st()))
        return self.y[:B]

    def backward(self, dy, B):
        rt = self.rt
        rt.ck(rt.lib.seld_pool2d_bwd(rt.p(dy), rt.p(self.idx), rt.p(self.dx), B, self.H, self.W, self.C, self.ph, self.pw, self.same, rt.st()))
        return self.dx[:B]


class BatchNorm:
    """tf.keras.layers.BatchNormalization() on the channel axis: batch statistics in training (moving statistics updated), the moving ones
    otherwise."""

    def __init__(self, rt: _Rt, name: str, shape, B: int):
        self.rt, self.name = rt, name
        self.H, self.W, self.C = shape
        rt.var(f"{name}.gamma", (self.C,))
        rt.var(f"{name}.beta", (self.C,))
        rt.var(f"{name}.moving_mean", (self.C,), trainable=False)
        rt.var(f"{name}.moving_variance", (self.C,), trainable=False)
        self.mean, self.var = rt.empty(self.C), rt.empty(self.C)
        self.scratch = rt.bn_scratch(self.C)

    def forward(self, z, out, B, training, accumulate):
        rt, n = self.rt, self.name
        npix = B * self.H * self.W
        self.z = z
        if training:
            rt.ck(rt.lib.seld_m_bn_stats(rt.p(z), npix, self.C, rt.p(self.mean), rt.p(self.var), rt.p(self.scratch), rt.st()))
            mean, var = self.mean, self.var
            rt.ck(rt.lib.seld_m_bn_moving(rt.p(mean), rt.p(var), rt.p(rt.w(f"{n}.moving_mean")), rt.p(rt.w(f"{n}.moving_variance")), self.C,
                                          BN_MOMENTUM, npix, rt.st()))
        else:
            mean, var = rt.w(f"{n}.moving_mean"), rt.w(f"{n}.moving_variance")
        rt.ck(rt.lib.seld_m_bn_apply(rt.p(z), rt.p(mean), rt.p(var), rt.p(rt.w(f"{n}.gamma")), rt.p(rt.w(f"{n}.beta")), BN_EPS, rt.p(out), npix,
                                     self.C, int(accumulate), rt.st()))

    def backward(self, dy, dz, B):
        rt, n = self.rt, self.name
        rt.ck(rt.lib.seld_m_bn_bwd(rt.p(self.z), rt.p(dy), rt.p(self.mean), rt.p(self.var), rt.p(rt.w(f"{n}.gamma")), BN_EPS, rt.p(dz),
                                   rt.p(rt.g(f"{n}.gamma")), rt.p(rt.g(f"{n}.beta")), B * self.H * self.W, self.C, rt.p(self.scratch), rt.st()))


class _ConvBN:
    """Conv2D + BatchNormalization: the pair every branch of mother_block is made of"""

    def __init__(self, rt, cname, bname, in_shape, filters, k, strides, B):
        self.conv = Conv2D(rt, cname, in_shape, filters, k, strides, B)
        self.bn = BatchNorm(rt, bname, self.conv.out_shape, B)
        self.out_shape = self.conv.out_shape
        self.dz = rt.empty(B, *self.out_shape)

    def forward(self, x, out, B, training, accumulate):
        self.bn.forward(self.conv.forward(x, B), out, B, training, accumulate)

    def backward(self, dy, dx, B, accumulate):
        self.bn.backward(dy, self.dz, B)
        self.conv.backward(self.dz, dx, B, accumulate)


class LayerNorm:
    """tf.keras.layers.LayerNormalization() over the last axis of [rows, C], with the residual sum in front of it folded in:
    forward(x, r) = LN(x + r) (r None: LN(x)); backward gives the gradient of the SUMMED input, which the caller routes to both addends."""

    def __init__(self, rt: _Rt, name: str, rows: int, C: int):
        self.rt, self.name, self.C = rt, name, int(C)
        rt.var(f"{name}.gamma", (self.C,))
        rt.var(f"{name}.beta", (self.C,))
        self.y, self.xhat, self.rstd, self.dz = rt.empty(rows, self.C), rt.empty(rows, self.C), rt.empty(rows), rt.empty(rows, self.C)
        self.scratch = rt.empty(int(rt.lib.seld_ln_scratch(rows, self.C)))

    def forward(self, x, r, rows, training):
        rt, n = self.rt, self.name
        rt.ck(rt.lib.seld_ln_fwd(rt.p(x), rt.p(r), rt.p(rt.w(f"{n}.gamma")), rt.p(rt.w(f"{n}.beta")), LN_EPS, rt.p(self.y),
                                 rt.p(self.xhat) if training else None, rt.p(self.rstd) if training else None, rows, self.C, rt.st()))
        return self.y[:rows]

    def backward(self, dy, rows):
        rt, n = self.rt, self.name
        rt.ck(rt.lib.seld_ln_bwd(rt.p(dy), rt.p(self.xhat), rt.p(self.rstd), rt.p(rt.w(f"{n}.gamma")), rt.p(self.dz), rt.p(rt.g(f"{n}.gamma")),
                                 rt.p(rt.g(f"{n}.beta")), rt.p(self.scratch), rows, self.C, rt.st()))
        return self.dz[:rows]


class _Attention:
    """What the three attention layers allocate alike on [B, S, D] with H heads of dk: q k v o do, the gradients dq dk_ dv, the softmax's lse,
    the backward kernel's scratch (`scratch_fn(B, S, H, dk)` floats; negative: the kernels refuse this key_dim), the output and the scale.
    any_width: the layer's core is seld_attn_*, which on a runtime with any_key_dim has a form for every dk in 1..64 (seld_attnw_*)."""
    any_width = False

    def __init__(self, rt: _Rt, name: str, B: int, S: int, D: int, n_head: int, key_dim: int, scratch_fn, drop: _Drop = None, site: int = 0):
        self.rt, self.name, self.S, self.D, self.H, self.dk = rt, name, int(S), int(D), int(n_head), int(key_dim)
        self.drop, self.site = drop, site      # the probabilities' Dropout (None: none)
        self.wide = self.any_width and rt.any_key_dim and self.dk % 8 != 0      # a multiple of 8 keeps the calls of every other runtime
        if self.wide:
            scratch_fn = rt.lib.seld_attnw_bwd_scratch
        need = int(scratch_fn(B, self.S, self.H, self.dk))
        if need < 0:
            raise ValueError(f"key_dim {key_dim!r}: the attention kernels take " +
                             ("an integer from 1 to 64" if self.wide else "a multiple of 8 from 8 to 64"))
        R, HD = B * self.S, self.H * self.dk
        self.q, self.k, self.v, self.o, self.do = (rt.empty(R, HD) for _ in range(5))
        self.dq, self.dk_, self.dv = (rt.empty(R, HD) for _ in range(3))
        self.lse = rt.empty(B * self.H * self.S)
        self.scratch = rt.empty(need)
        self.out = rt.empty(R, self.D)
        self.scale = 1.0 / math.sqrt(float(self.dk))

    def _core_fwd(self, B, training):
        """o = softmax(scale q k^T) v per head (seld_attn_fwd), the probabilities dropped where the block's Dropout draws (seld_attn_drop_fwd);
        a dk that is no multiple of 8 (`wide`): seld_attnw_fwd / seld_attnw_drop_fwd"""
        rt, HD = self.rt, self.H * self.dk
        args = (rt.p(self.q), rt.p(self.k), rt.p(self.v), HD, HD, HD, rt.p(self.o), rt.p(self.lse) if training else None, B, self.S, self.H, self.dk,
                self.scale)
        lib = rt.lib
        if self.drop is not None and self.drop.on:
            fn = lib.seld_attnw_drop_fwd if self.wide else lib.seld_attn_drop_fwd
            rt.ck(fn(*args, self.drop.rate, rt.dropout_seed, self.drop.base + self.site, rt.dropout_cur, rt.st()))
        else:
            rt.ck((lib.seld_attnw_fwd if self.wide else lib.seld_attn_fwd)(*args, rt.st()))

    def _core_bwd(self, B):
        """dq, dk_, dv from do (seld_attn_bwd / seld_attn_drop_bwd with the forward's masks; `wide`: seld_attnw_bwd / seld_attnw_drop_bwd)"""
        rt, HD = self.rt, self.H * self.dk
        args = (rt.p(self.q), rt.p(self.k), rt.p(self.v), HD, HD, HD, rt.p(self.o), rt.p(self.do), rt.p(self.lse), rt.p(self.dq), rt.p(self.dk_),
                rt.p(self.dv), HD, HD, HD, rt.p(self.scratch), B, self.S, self.H, self.dk, self.scale)
        lib = rt.lib
        if self.drop is not None and self.drop.on:
            fn = lib.seld_attnw_drop_bwd if self.wide else lib.seld_attn_drop_bwd
            rt.ck(fn(*args, self.drop.rate, rt.dropout_seed, self.drop.base + self.site, rt.dropout_cur, rt.st()))
        else:
            rt.ck((lib.seld_attnw_bwd if self.wide else lib.seld_attn_bwd)(*args, rt.st()))


class MultiHeadAttention(_Attention):
    """tf.keras.layers.MultiHeadAttention(n_head, key_dim, dropout)(x, x) on [B, S, D] (value_dim = key_dim, biases): three projections
    (one seld_m_gemm each: Keras' kernels [D, H, dk] are [D, H dk] row-major), the query scaled by 1 / sqrt(key_dim), seld_attn_fwd (in
    training with `drop`: seld_attn_drop_fwd), and the output projection [H dk, D]."""
    any_width = True

    def __init__(self, rt: _Rt, name: str, B: int, S: int, D: int, n_head: int, key_dim: int, drop: _Drop = None, site: int = 0):
        super().__init__(rt, name, B, S, D, n_head, key_dim, rt.lib.seld_attn_bwd_scratch, drop, site)
        H, dk = self.H, self.dk
        for part in ("query", "key", "value"):
            rt.var(f"{name}.{part}.kernel", (self.D, H, dk))
            rt.var(f"{name}.{part}.bias", (H, dk))
        rt.var(f"{name}.attention_output.kernel", (H, dk, self.D))
        rt.var(f"{name}.attention_output.bias", (self.D,))

    def forward(self, x, B, training):
        rt, n = self.rt, self.name
        R, HD = B * self.S, self.H * self.dk
        self.x = x
        for part, buf in (("query", self.q), ("key", self.k), ("value", self.v)):
            rt.gemm(x, rt.w(f"{n}.{part}.kernel"), rt.w(f"{n}.{part}.bias"), buf, R, HD, self.D)
        self._core_fwd(B, training)
        rt.gemm(self.o, rt.w(f"{n}.attention_output.kernel"), rt.w(f"{n}.attention_output.bias"), self.out, R, self.D, HD)
        return self.out[:R]

    def backward(self, dout, dx, B):
        """dout [R, D] -> every variable's gradient; dx = the input's gradient (overwritten)"""
        rt, n = self.rt, self.name
        R, HD = B * self.S, self.H * self.dk
        rt.gemm_tn(self.o, dout, rt.g(f"{n}.attention_output.kernel"), rt.g(f"{n}.attention_output.bias"), R, HD, self.D)
        rt.gemm(dout, rt.w(f"{n}.attention_output.kernel"), None, self.do, R, HD, self.D, transb=1)
        self._core_bwd(B)
        for i, (part, g) in enumerate((("query", self.dq), ("key", self.dk_), ("value", self.dv))):
            rt.gemm_tn(self.x, g, rt.g(f"{n}.{part}.kernel"), rt.g(f"{n}.{part}.bias"), R, self.D, HD)
            rt.gemm(g, rt.w(f"{n}.{part}.kernel"), None, dx, R, self.D, HD, transb=1, accumulate=int(i > 0))


class Conv1D(Linear):
    """tf.keras.layers.Conv1D(filters, k, padding='same') over the frames of [rows, Cin], rows = B * S: seld_m_im2col with a (k, 1) window
    (skipped for k = 1) + the MFMA GEMM over the K = k Cin columns; kernel [k, Cin, filters]."""

    def __init__(self, rt: _Rt, name: str, B: int, S: int, Cin: int, filters: int, k: int):
        self.S, self.Cin, self.k = int(S), int(Cin), int(k)
        super().__init__(rt, name, B * self.S, self.k * self.Cin, filters, (self.k, self.Cin, int(filters)))
        self.col = self.dcol = None
        if self.k > 1:
            self.col, self.dcol = rt.empty(B * self.S, self.K), rt.empty(B * self.S, self.K)

    def forward(self, x, rows):
        rt = self.rt
        if self.k > 1:
            rt.ck(rt.lib.seld_m_im2col(rt.p(x), rt.p(self.col), rows // self.S, self.S, 1, self.Cin, self.k, 1, 1, 1, rt.st()))
            x = self.col
        return Linear.forward(self, x, rows)

    def backward(self, dz, dx, rows):
        rt = self.rt
        if self.k == 1:
            return Linear.backward(self, dz, dx, rows)
        Linear.backward(self, dz, self.dcol, rows)
        rt.ck(rt.lib.seld_m_col2im(rt.p(self.dcol), rt.p(dx), rows // self.S, self.S, 1, self.Cin, self.k, 1, 1, 1, 0, rt.st()))


class _FeedForward:
    """second(act(first(x))) on [rows, D], first / second two Linear layers (Dense or Conv1D) that the owner built: the hidden buffer h, and
    a backward that takes the output's gradient (times `factor`, the owner's residual scale, where one is given) to the input's.  `scratch`:
    the backward buffers (dh, dpre[, df]) of an owner that shares them among its cores; None: this core's own.  `drop` / `sites`: the owner's
    Dropout and the sites of the two Dropout layers of the reference's FFNs — behind the activation (applied here, in place on h) and behind
    the second layer (the OWNER applies it, with its residual sum: drop.add; the backward here masks the incoming gradient)."""

    def __init__(self, rt: _Rt, first: Linear, second: Linear, rows: int, act: int, factor=None, scratch=None, drop: _Drop = None, sites=(0, 1)):
        self.rt, self.first, self.second, self.act, self.factor = rt, first, second, act, factor
        self.drop, self.sites = drop, sites
        self.h = rt.empty(rows, first.N)
        self.dh, self.dpre, self.df = scratch or (rt.empty(rows, first.N), rt.empty(rows, first.N), None)
        if (factor is not None or (drop is not None and drop.rate > 0)) and self.df is None:
            self.df = rt.empty(rows, second.N)

    def hidden(self, x, rows):
        """Dropout(act(first(x))): for an owner that has something to launch between the two layers; forward() otherwise"""
        self.pre = self.first.forward(x, rows)
        h = self.h[:rows]
        self.rt.act(self.pre, h, self.act)
        if self.drop is not None and self.drop.on:
            self.drop.apply(self.sites[0], h, h)
        return h

    def forward(self, x, rows):
        return self.second.forward(self.hidden(x, rows), rows)

    def backward(self, dy, dx, rows):
        """dy [rows, D]: the gradient of the (scaled) output, behind its Dropout -> dx = the input's gradient (overwritten)"""
        rt = self.rt
        on = self.drop is not None and self.drop.on
        if on:
            dy = self.drop.apply(self.sites[1], dy, self.df[:rows], 1.0 if self.factor is None else self.factor)
        elif self.factor is not None:
            df = self.df[:rows]
            df.zero_()
            rt.axpy(df, dy, self.factor)
            dy = df
        self.second.backward(dy, self.dh[:rows], rows)
        if on:
            self.drop.apply(self.sites[0], self.dh[:rows], self.dh[:rows])
        rt.act_bwd(self.pre, self.dh[:rows], self.dpre[:rows], self.act)
        self.first.backward(self.dpre[:rows], dx, rows)


class Stage:
    """`depth` blocks of one kind in a row (reference modules.py:64-83, 106-180: the *_stage functions; a *_block is a stage of one): every
    block is `block(rt, cfg, S, D, prefix + index, B)` with forward(x, B, training) / backward(dy, B) on [B*S, D] -> [B*S, out_dim], and
    reads the width the one in front of it gives (behind an RNN_block with merge_mode 'concat': 256)."""

    def __init__(self, rt: _Rt, block, cfg: dict, S: int, D: int, prefix: str, B: int, depth: int, first_block: int = 0):
        """first_block: the blocks a chain of stages built in front of this one (ConvTemporalNet); its blocks draw from the streams
        DROP_STREAM0 + 32 * (first_block + index), so that two stages of one model never share masks.  models.seldnet has one stage: 0."""
        self.blocks = []
        self.rt, self.S, self.D = rt, int(S), int(D)
        self.model = False      # True: this stage IS the model (a factory built it on a runtime of its own), so its training forwards count the draws
        for i in range(int(depth)):
            self.blocks.append(block(rt, cfg, S, D, f"{prefix}{i}", B, **({"layer": i} if getattr(block, "PER_LAYER_UNITS", False) else {})))
            D = self.blocks[-1].out_dim
            if getattr(self.blocks[-1], "drop", None) is not None:
                self.blocks[-1].drop.base = DROP_STREAM0 + 32 * (int(first_block) + i)
        self.out_dim, self.out_shape = int(D), (self.S, int(D))

    def forward(self, x, B, training):
        if self.model and training:
            self.rt.next_draws()
        for blk in self.blocks:
            x = blk.forward(x, B, training)
        return x

    def backward(self, dy, B):
        for blk in reversed(self.blocks):
            dy = blk.backward(dy, B)
        return dy


TRANSFORMER_KEYS = ("n_head", "key_dim", "ff_multiplier", "kernel_size")


def check_transformer_config(cfg: dict, stage: bool = False, dropout: bool = False, any_key_dim: bool = False) -> None:
    """the mandatory keys of reference modules.py:380-383 (and `depth`, modules.py:120); what has no kernel here is refused, not ignored.
    any_key_dim: key_dim may be any integer in 1..64 (seld_attnw_*), not only a multiple of 8"""
    for key in TRANSFORMER_KEYS + (("depth",) if stage else ()):
        if key not in cfg:
            raise ValueError(f"transformer_encoder_{'stage' if stage else 'block'}: missing {key!r}")
    _check_activation(cfg, "relu")
    _dropout_rate(cfg, "transformer_encoder_block", dropout)
    if int(cfg["n_head"]) < 1 or int(cfg["kernel_size"]) < 1 or float(cfg["ff_multiplier"]) <= 0 or (stage and int(cfg["depth"]) < 1):
        raise ValueError("transformer_encoder_block: n_head, kernel_size, depth >= 1 and ff_multiplier > 0")
    _check_key_dim(cfg["key_dim"], any_key_dim)


class TransformerEncoderBlock:
    """reference modules.transformer_encoder_block (modules.py:379-407) on [B, S, D]:
    x = LN(x + Dropout(MHA(x, x))); ffn = Dropout(Conv1D(D, k)(Dropout(Conv1D(int(ff_multiplier D), k, activation)(x)))); x = LN(x + ffn);
    the MultiHeadAttention drops its probabilities at the same rate.  The Dropouts draw in training only (_Drop: sites 0 - 3)."""

    def __init__(self, rt: _Rt, cfg: dict, S: int, D: int, prefix: str, B: int):
        check_transformer_config(cfg, dropout=rt.dropout, any_key_dim=rt.any_key_dim)
        self.rt, self.S, self.D, self.B = rt, int(S), int(D), B
        self.F = int(cfg["ff_multiplier"] * self.D)
        if self.F < 1:
            raise ValueError("transformer_encoder_block: int(ff_multiplier * d_model) < 1")
        k = int(cfg["kernel_size"])
        R = B * self.S
        self.drop = _Drop(rt, _dropout_rate(cfg, "transformer_encoder_block", rt.dropout))
        self.mha = MultiHeadAttention(rt, f"{prefix}.mha", B, self.S, self.D, int(cfg["n_head"]), int(cfg["key_dim"]), self.drop, 0)
        self.ln0 = LayerNorm(rt, f"{prefix}.ln0", R, self.D)
        self.ffn = _FeedForward(rt, Conv1D(rt, f"{prefix}.ffn0", B, self.S, self.D, self.F, k), Conv1D(rt, f"{prefix}.ffn1", B, self.S, self.F, self.D, k),
                                R, ACT[cfg.get("activation", "relu")], drop=self.drop, sites=(2, 3))
        self.ln1 = LayerNorm(rt, f"{prefix}.ln1", R, self.D)
        self.dx1, self.dx = rt.empty(R, self.D), rt.empty(R, self.D)
        self.dd = rt.empty(R, self.D) if self.drop.rate > 0 else None      # a gradient behind a Dropout
        self.out_dim, self.out_shape = self.D, (self.S, self.D)

    def forward(self, x, B, training):
        """x [B*S, D] (or any contiguous view of it) -> [B*S, D]"""
        R = B * self.S
        x = x.reshape(R, self.D)
        drop = self.drop
        drop.begin(training)
        attn = self.mha.forward(x, B, training)
        if drop.on:
            drop.apply(1, attn, attn)
        x1 = self.ln0.forward(attn, x, R, training)
        ffn = self.ffn.forward(x1, R)
        if drop.on:
            drop.apply(3, ffn, ffn)
        return self.ln1.forward(ffn, x1, R, training)

    def backward(self, dy, B):
        """dy [B*S, D]: the output's gradient -> the input's gradient [B*S, D] (a buffer of this block)"""
        rt = self.rt
        R = B * self.S
        dz1 = self.ln1.backward(dy.reshape(R, self.D), R)          # gradient of x1 + ffn
        dx1 = self.dx1[:R]
        self.ffn.backward(dz1, dx1, R)
        rt.axpy(dx1, dz1)
        dz0 = self.ln0.backward(dx1, R)                             # gradient of x + attn
        dx = self.dx[:R]
        self.mha.backward(self.drop.apply(1, dz0, self.dd[:R]) if self.drop.on else dz0, dx, B)
        rt.axpy(dx, dz0)
        return dx


class _HeadMajorAttention(_Attention):
    """What the reference's own two attention layers share (layers.py:102-287, 332-392; not Keras' layer): head-major kernels query_kernel /
    key_kernel / value_kernel [H, D, dk] and projection_kernel [H, dk, D], then (use_bias) projection_bias [D] and q_bias / k_bias / v_bias
    [H, dk] — created in that order.  The variables keep the reference's layout; seld_head_permute packs a kernel to the [D, H dk] matrix of a
    GEMM in front of each forward and unpacks its gradient behind each backward.  The query's division by sqrt(dk) (layers.py:275-276, after
    the bias) is the core kernel's `scale`."""
    PARTS = ("query", "key", "value")

    def __init__(self, rt: _Rt, name: str, B: int, S: int, D: int, n_head: int, key_dim: int, use_bias: bool, scratch_fn, n_packed: int = 3,
                 drop: _Drop = None, site: int = 0):
        super().__init__(rt, name, B, S, D, n_head, key_dim, scratch_fn, drop, site)
        self.use_bias = bool(use_bias)
        H, dk = self.H, self.dk
        for part in self.PARTS:
            rt.var(f"{name}.{part}_kernel", (H, self.D, dk))
        rt.var(f"{name}.projection_kernel", (H, dk, self.D))
        if self.use_bias:
            rt.var(f"{name}.projection_bias", (self.D,))
            for part in "qkv":
                rt.var(f"{name}.{part}_bias", (H, dk))
        self.packed = [rt.empty(self.D, H * dk) for _ in range(n_packed)]      # query, key, value (, pos)
        self.dpacked = rt.empty(self.D, H * dk)

    def _bias(self, part, grad=False):
        if not self.use_bias:
            return None
        return (self.rt.g if grad else self.rt.w)(f"{self.name}.{part}")

    def _pack(self, kernel, wp):
        rt = self.rt
        rt.ck(rt.lib.seld_head_permute(rt.p(rt.w(f"{self.name}.{kernel}")), rt.p(wp), self.H, self.D, self.dk, 0, rt.st()))

    def _unpack(self, kernel):
        """dpacked [D, H dk] -> the gradient of `kernel` [H, D, dk]"""
        rt = self.rt
        rt.ck(rt.lib.seld_head_permute(rt.p(self.dpacked), rt.p(rt.g(f"{self.name}.{kernel}")), self.H, self.D, self.dk, 1, rt.st()))

    def _qkv(self, x, R):
        self.x = x
        for part, wp, buf in zip(self.PARTS, self.packed, (self.q, self.k, self.v)):
            self._pack(f"{part}_kernel", wp)
            self.rt.gemm(x, wp, self._bias(part[0] + "_bias"), buf, R, self.H * self.dk, self.D)

    def _project(self, R):
        rt = self.rt
        rt.gemm(self.o, rt.w(f"{self.name}.projection_kernel"), self._bias("projection_bias"), self.out, R, self.D, self.H * self.dk)
        return self.out[:R]

    def _project_bwd(self, dout, R):
        """dout [R, D] -> the projection's gradients and do"""
        rt, HD = self.rt, self.H * self.dk
        rt.gemm_tn(self.o, dout, rt.g(f"{self.name}.projection_kernel"), self._bias("projection_bias", True), R, HD, self.D)
        rt.gemm(dout, rt.w(f"{self.name}.projection_kernel"), None, self.do, R, HD, self.D, transb=1)

    def _input_bwd(self, i, g, dx, R, accumulate):
        """g: the gradient of q, k or v (i = 0, 1, 2) -> its kernel's and bias's gradients; dx (+)= g kernel^T"""
        rt, part, HD = self.rt, self.PARTS[i], self.H * self.dk
        rt.gemm_tn(self.x, g, self.dpacked, self._bias(part[0] + "_bias", True), R, self.D, HD)
        self._unpack(f"{part}_kernel")
        rt.gemm(g, self.packed[i], None, dx, R, self.D, HD, transb=1, accumulate=accumulate)


class MultiHeadAttentionRef(_HeadMajorAttention):
    """The reference's layers.MultiHeadAttention_(n_head, key_dim, use_bias, dropout)([x, x, x]) (layers.py:102-287) on [B, S, D]: seld_attn_fwd /
    _bwd (in training with `drop`, the probabilities' Dropout of layers.py:253-257: seld_attn_drop_fwd / _bwd) between the shared projections."""
    any_width = True

    def __init__(self, rt: _Rt, name: str, B: int, S: int, D: int, n_head: int, key_dim: int, use_bias: bool = True, drop: _Drop = None,
                 site: int = 0):
        super().__init__(rt, name, B, S, D, n_head, key_dim, use_bias, rt.lib.seld_attn_bwd_scratch, drop=drop, site=site)

    def forward(self, x, B, training):
        R = B * self.S
        self._qkv(x, R)
        self._core_fwd(B, training)
        return self._project(R)

    def backward(self, dout, dx, B):
        """dout [R, D] -> every variable's gradient; dx = the input's gradient (overwritten)"""
        R = B * self.S
        self._project_bwd(dout, R)
        self._core_bwd(B)
        for i, g in enumerate((self.dq, self.dk_, self.dv)):
            self._input_bwd(i, g, dx, R, accumulate=int(i > 0))


class DepthwiseConv1D:
    """[GLU +] tf.keras.layers.Conv1D(filters=C, kernel_size=k, strides=1, padding='same', groups=C) over the frames of [B, S, C]
    (modules.py:476-486): seld_dwconv1d_fwd / _bwd.  glu: the input is [B*S, 2C] and a * sigmoid(b) is formed inside the kernel.
    Keras' kernel [k, 1, C] and bias [C]."""

    def __init__(self, rt: _Rt, name: str, B: int, S: int, C_: int, k: int, glu: bool = True):
        self.rt, self.name, self.S, self.C, self.k, self.glu = rt, name, int(S), int(C_), int(k), int(bool(glu))
        rt.var(f"{name}.kernel", (self.k, 1, self.C))
        rt.var(f"{name}.bias", (self.C,))
        need = int(rt.lib.seld_dwconv1d_bwd_scratch(B, self.S, self.C, self.k))
        if need < 0:
            raise ValueError(f"depthwise Conv1D: kernel_size {k!r} (1 .. 64), B {B}, S {S}, C {C_} are refused by the kernels")
        self.scratch = rt.empty(need)
        self.y = rt.empty(B * self.S, self.C)

    def forward(self, u, B):
        rt, n = self.rt, self.name
        self.u = u
        rt.ck(rt.lib.seld_dwconv1d_fwd(rt.p(u), (1 + self.glu) * self.C, rt.p(rt.w(f"{n}.kernel")), rt.p(rt.w(f"{n}.bias")), rt.p(self.y), B, self.S,
                                       self.C, self.k, self.glu, rt.st()))
        return self.y[:B * self.S]

    def backward(self, dy, du, B):
        rt, n = self.rt, self.name
        ld = (1 + self.glu) * self.C
        rt.ck(rt.lib.seld_dwconv1d_bwd(rt.p(self.u), ld, rt.p(rt.w(f"{n}.kernel")), rt.p(dy), rt.p(du), ld, rt.p(rt.g(f"{n}.kernel")),
                                       rt.p(rt.g(f"{n}.bias")), rt.p(self.scratch), B, self.S, self.C, self.k, self.glu, rt.st()))


class _ConvTail:
    """The convolution module's tail (reference modules.py:476-493, 603-613): depthwise Conv1D(k) [on the GLU of a 2 D wide input] ->
    BatchNormalization -> swish -> pointwise Conv1D(D, 1), variables `{prefix}.dw`, `.bn`, `.pw1` in that order.  What sits in front of it
    (LayerNormalization, the pointwise Conv1D(2 D, 1) of the GLU) and the residual behind it are the owning block's."""

    def __init__(self, rt: _Rt, prefix: str, B: int, S: int, D: int, k: int, glu: bool):
        self.rt, self.S = rt, int(S)
        self.dw = DepthwiseConv1D(rt, f"{prefix}.dw", B, S, D, k, glu=glu)
        self.bn = BatchNorm(rt, f"{prefix}.bn", (S, 1, D), B)
        self.pw1 = Conv1D(rt, f"{prefix}.pw1", B, S, D, D, 1)
        self.bno, self.sw, self.dsw, self.dbn, self.ddw = (rt.empty(B * S, D) for _ in range(5))

    def hidden(self, c, B, training):
        """swish(BN(depthwise(c))): for an owner that has something to launch in front of the pointwise layer; forward() otherwise"""
        rt, R = self.rt, B * self.S
        self.bn.forward(self.dw.forward(c, B), self.bno[:R], B, training, 0)
        rt.act(self.bno[:R], self.sw[:R], ACT["swish"])
        return self.sw[:R]

    def forward(self, c, B, training):
        return self.pw1.forward(self.hidden(c, B, training), B * self.S)

    def backward(self, dy, du, B):
        """dy [B*S, D]: the output's gradient -> du = the gradient of the depthwise convolution's input (overwritten)"""
        rt, R = self.rt, B * self.S
        self.pw1.backward(dy, self.dsw[:R], R)
        rt.act_bwd(self.bno[:R], self.dsw[:R], self.dbn[:R], ACT["swish"])
        self.bn.backward(self.dbn[:R], self.ddw[:R], B)
        self.dw.backward(self.ddw[:R], du, B)


def basic_pos_encoding(S: int, D: int) -> np.ndarray:
    """layers.basic_pos_encoding (layers.py:53-67) as a [S, D] float32 table: column 2 i = cos(w_i t), column 2 i + 1 = sin(w_i t), w_i =
    float32(10000 ** (-i / (D // 2))).  The product w t, cos and sin are taken in float64 and rounded once (TensorFlow forms w t in float32:
    DESIGN.md section 3f)."""
    k = int(D) // 2
    w = np.power(10000.0, -np.arange(k, dtype=np.float64) / k).astype(np.float32).astype(np.float64)
    arg = np.arange(int(S), dtype=np.float64)[:, None] * w[None, :]
    return np.stack([np.cos(arg), np.sin(arg)], -1).reshape(int(S), 2 * k).astype(np.float32)


def check_conformer_config(cfg: dict, stage: bool = False, D=None, dropout: bool = False, any_key_dim: bool = False) -> None:
    """what reference modules.py:410-430 reads (every key has a default there; `depth` is the stage's, modules.py:146); what has no kernel
    here is refused, not ignored.  any_key_dim: key_dim may be any integer in 1..64 (seld_attnw_*), not only a multiple of 8"""
    who = f"conformer_encoder_{'stage' if stage else 'block'}"
    if stage and "depth" not in cfg:
        raise ValueError(f"{who}: missing 'depth'")
    _check_activation(cfg, "swish")
    _dropout_rate(cfg, who, dropout)
    if cfg.get("pos_mode", "absolute") != "absolute":
        raise ValueError(f"{who}: pos_mode {cfg.get('pos_mode')!r}: RelPositionMultiHeadAttention has no kernel here, only 'absolute'")
    _check_pos_encoding(cfg, who, D)
    reg = cfg.get("kernel_regularizer", None)
    if reg is not None and (not isinstance(reg, dict) or set(reg) - {"l1", "l2"}):
        raise ValueError(f"{who}: kernel_regularizer {reg!r}: a dict of l1 / l2 (it only feeds model.losses, which train.trainstep never adds)")
    if int(cfg.get("n_head", 4)) < 1 or not 1 <= int(cfg.get("kernel_size", 32)) <= 64 or int(cfg.get("multiplier", 4)) < 1 or \
            (stage and int(cfg["depth"]) < 1):
        raise ValueError(f"{who}: n_head, multiplier, depth >= 1 and 1 <= kernel_size <= 64")
    _check_key_dim(cfg.get("key_dim", 36), any_key_dim)


class ConformerEncoderBlock:
    """reference modules.conformer_encoder_block (modules.py:432-506) on [B, S, D].  In training with dropout_rate > 0 the seven Dropouts draw
    (_Drop: behind each FFN's activation and output, on the attention probabilities, behind the attention and behind the convolution module);
    written without them:
      x  = x + ffn_factor Dense(D)(act(Dense(multiplier D)(LN(x))));  x = x + encoding (pos_encoding 'basic')
      x  = x + MultiHeadAttention_(LN(x))
      x' = x + Conv1D(D, 1)(swish(BN(depthwise Conv1D(k)(GLU(Conv1D(2 D, 1)(LN(x)))))))
      out = LN(x + ffn_factor Dense(D)(act(Dense(multiplier D)(LN(x')))))       — the last residual adds to x, not x' (modules.py:495, 504)."""

    def __init__(self, rt: _Rt, cfg: dict, S: int, D: int, prefix: str, B: int):
        check_conformer_config(cfg, D=D, dropout=rt.dropout, any_key_dim=rt.any_key_dim)
        self.rt, self.S, self.D, self.B = rt, int(S), int(D), B
        S, D = self.S, self.D
        self.F = int(cfg.get("multiplier", 4)) * D
        self.ff = float(cfg.get("ffn_factor", 0.5))
        R = B * S
        p = prefix
        e = rt.empty
        scratch = (e(R, self.F), e(R, self.F), e(R, D))      # dh, dpre, df: the two FFNs run one after the other
        self.drop = _Drop(rt, _dropout_rate(cfg, "conformer_encoder_block", rt.dropout))

        def ffn(name, sites):
            return _FeedForward(rt, Dense(rt, f"{name}a", R, D, self.F), Dense(rt, f"{name}b", R, self.F, D), R, ACT[cfg.get("activation", "swish")],
                                self.ff, scratch, self.drop, sites)
        self.ln0 = LayerNorm(rt, f"{p}.ln0", R, D)
        self.ffn0 = ffn(f"{p}.ffn0", (0, 1))
        self.ln1 = LayerNorm(rt, f"{p}.ln1", R, D)
        self.mha = MultiHeadAttentionRef(rt, f"{p}.mha", B, S, D, int(cfg.get("n_head", 4)), int(cfg.get("key_dim", 36)), cfg.get("use_bias", True),
                                         self.drop, 2)
        self.ln2 = LayerNorm(rt, f"{p}.ln2", R, D)
        self.pw0 = Conv1D(rt, f"{p}.pw0", B, S, D, 2 * D, 1)
        self.tail = _ConvTail(rt, p, B, S, D, int(cfg.get("kernel_size", 32)), glu=True)
        self.ln3 = LayerNorm(rt, f"{p}.ln3", R, D)
        self.ffn1 = ffn(f"{p}.ffn1", (5, 6))
        self.ln4 = LayerNorm(rt, f"{p}.ln4", R, D)
        self.enc = None
        if cfg.get("pos_encoding", "basic") == "basic":
            self.enc = torch.as_tensor(basic_pos_encoding(S, D)).to(rt.dev)
        self.x1, self.x2, self.x3, self.z = e(R, D), e(R, D), e(R, D), e(R, D)
        self.du = e(R, 2 * D)
        self.dx2, self.dx1, self.dx0, self.dn = e(R, D), e(R, D), e(R, D), e(R, D)
        self.dd = e(R, D) if self.drop.rate > 0 else None      # a gradient behind a Dropout
        self.out_dim, self.out_shape = D, (S, D)

    def _ffn_bwd(self, ln, ffn, dy, rows):
        """dy: the gradient of ffn_factor * the FFN's output -> the gradient of the input of its LayerNormalization"""
        ffn.backward(dy, self.dn[:rows], rows)
        return ln.backward(self.dn[:rows], rows)

    def forward(self, x, B, training):
        """x [B*S, D] (or any contiguous view of it) -> [B*S, D]"""
        rt = self.rt
        R, D = B * self.S, self.D
        x = x.reshape(R, D)
        x1, x2, x3, z = self.x1[:R], self.x2[:R], self.x3[:R], self.z[:R]
        drop = self.drop
        drop.begin(training)
        x1.copy_(x)
        drop.add(1, x1, self.ffn0.forward(self.ln0.forward(x, None, R, training), R), self.ff)
        if self.enc is not None:
            rt.ck(rt.lib.seld_pos_add(rt.p(x1), rt.p(self.enc), B, self.S, D, rt.st()))
        x2.copy_(x1)
        drop.add(3, x2, self.mha.forward(self.ln1.forward(x1, None, R, training), B, training))
        sw = self.tail.hidden(self.pw0.forward(self.ln2.forward(x2, None, R, training), R), B, training)
        x3.copy_(x2)
        drop.add(4, x3, self.tail.pw1.forward(sw, R))
        z.copy_(x2)
        drop.add(6, z, self.ffn1.forward(self.ln3.forward(x3, None, R, training), R), self.ff)
        return self.ln4.forward(z, None, R, training)

    def backward(self, dy, B):
        """dy [B*S, D]: the output's gradient -> the input's gradient [B*S, D] (a buffer of this block)"""
        rt = self.rt
        R, D = B * self.S, self.D
        dx2, dx1, dx0 = self.dx2[:R], self.dx1[:R], self.dx0[:R]
        dz = self.ln4.backward(dy.reshape(R, D), R)                      # gradient of x2 + ffn_factor ffn1
        dx2.copy_(dz)
        dx3 = self._ffn_bwd(self.ln3, self.ffn1, dz, R)                  # gradient of x3 = x2 + conv
        rt.axpy(dx2, dx3)
        self.tail.backward(self.drop.apply(4, dx3, self.dd[:R]) if self.drop.on else dx3, self.du[:R], B)
        self.pw0.backward(self.du[:R], self.dn[:R], R)
        rt.axpy(dx2, self.ln2.backward(self.dn[:R], R))
        dx1.copy_(dx2)
        self.mha.backward(self.drop.apply(3, dx2, self.dd[:R]) if self.drop.on else dx2, self.dn[:R], B)
        rt.axpy(dx1, self.ln1.backward(self.dn[:R], R))
        dx0.copy_(dx1)                                                   # the positional table is a constant
        rt.axpy(dx0, self._ffn_bwd(self.ln0, self.ffn0, dx1, R))
        return dx0


class GLU:
    """tf.split(u, 2, -1); u_1 * sigmoid(u_2) on [rows, 2C] (reference modules.py:599-601: attention_block's GLU without a depthwise
    convolution behind it): seld_glu_fwd / _bwd."""

    def __init__(self, rt: _Rt, rows: int, C_: int):
        self.rt, self.C = rt, int(C_)
        self.y = rt.empty(rows, self.C)

    def forward(self, u, rows):
        rt = self.rt
        self.u = u
        rt.ck(rt.lib.seld_glu_fwd(rt.p(u), 2 * self.C, rt.p(self.y), rows, self.C, rt.st()))
        return self.y[:rows]

    def backward(self, dy, du, rows):
        rt = self.rt
        rt.ck(rt.lib.seld_glu_bwd(rt.p(self.u), 2 * self.C, rt.p(dy), rt.p(du), 2 * self.C, rows, self.C, rt.st()))


class RelPositionMultiHeadAttention(_HeadMajorAttention):
    """The reference's layers.RelPositionMultiHeadAttention(n_head, key_dim, use_bias)([x, x, x, pos]) (layers.py:332-392) on [B, S, D] with the
    batch-free table pos [S, D] of layers.basic_pos_encoding: variables pos_kernel [H, D, dk], pos_bias_u, pos_bias_v [H, dk], then
    MultiHeadAttention_'s (layers.py:333-357, 148-205).  P = pos . pos_kernel is seld_head_permute + one GEMM as q, k, v are (from the
    host-built table in every forward: the kernel moves); the core is seld_relattn_fwd / _bwd, whose dQu (`dq`) / dQv are added for the query's
    gradient and column-summed for the two biases; dpos_kernel = pos^T dP."""

    def __init__(self, rt: _Rt, name: str, B: int, S: int, D: int, n_head: int, key_dim: int, use_bias: bool = False):
        rt.var(f"{name}.pos_kernel", (int(n_head), int(D), int(key_dim)))
        rt.var(f"{name}.pos_bias_u", (int(n_head), int(key_dim)))
        rt.var(f"{name}.pos_bias_v", (int(n_head), int(key_dim)))
        super().__init__(rt, name, B, S, D, n_head, key_dim, use_bias, rt.lib.seld_relattn_bwd_scratch, n_packed=4)
        HD = self.H * self.dk
        self.dqv, self.dpacked2 = rt.empty(B * self.S, HD), rt.empty(self.D, HD)
        self.P, self.dP = rt.empty(self.S, HD), rt.empty(self.S, HD)
        self.pos = torch.as_tensor(basic_pos_encoding(self.S, self.D)).to(rt.dev)

    def forward(self, x, B, training):
        rt, n = self.rt, self.name
        R, HD = B * self.S, self.H * self.dk
        self._qkv(x, R)
        self._pack("pos_kernel", self.packed[3])
        rt.gemm(self.pos, self.packed[3], None, self.P, self.S, HD, self.D)
        rt.ck(rt.lib.seld_relattn_fwd(rt.p(self.q), rt.p(self.k), rt.p(self.v), HD, HD, HD, rt.p(self.P), HD, rt.p(rt.w(f"{n}.pos_bias_u")),
                                      rt.p(rt.w(f"{n}.pos_bias_v")), rt.p(self.o), rt.p(self.lse) if training else None, B, self.S, self.H,
                                      self.dk, self.scale, rt.st()))
        return self._project(R)

    def backward(self, dout, dx, B):
        """dout [R, D] -> every variable's gradient; dx = the input's gradient (overwritten)"""
        rt, n = self.rt, self.name
        R, HD = B * self.S, self.H * self.dk
        self._project_bwd(dout, R)
        rt.ck(rt.lib.seld_relattn_bwd(rt.p(self.q), rt.p(self.k), rt.p(self.v), HD, HD, HD, rt.p(self.P), HD, rt.p(rt.w(f"{n}.pos_bias_u")),
                                      rt.p(rt.w(f"{n}.pos_bias_v")), rt.p(self.o), rt.p(self.do), rt.p(self.lse), rt.p(self.dq), rt.p(self.dqv),
                                      rt.p(self.dk_), rt.p(self.dv), rt.p(self.dP), HD, HD, HD, HD, HD, rt.p(self.scratch), B, self.S, self.H,
                                      self.dk, self.scale, rt.st()))
        # the query kernel sees dQu + dQv; the column sums of the two parts are the gradients of pos_bias_u / pos_bias_v
        rt.gemm_tn(self.x, self.dq, self.dpacked, rt.g(f"{n}.pos_bias_u"), R, self.D, HD)
        rt.gemm_tn(self.x, self.dqv, self.dpacked2, rt.g(f"{n}.pos_bias_v"), R, self.D, HD)
        rt.axpy(self.dpacked, self.dpacked2)
        self._unpack("query_kernel")
        if self.use_bias:
            gq = rt.g(f"{n}.q_bias")
            gq.copy_(rt.g(f"{n}.pos_bias_u"))
            rt.axpy(gq, rt.g(f"{n}.pos_bias_v"))
        dq = self.dq[:R]
        rt.axpy(dq, self.dqv[:R])
        rt.gemm(dq, self.packed[0], None, dx, R, self.D, HD, transb=1)
        for i, g in ((1, self.dk_), (2, self.dv)):
            self._input_bwd(i, g, dx, R, accumulate=1)
        rt.gemm_tn(self.pos, self.dP, self.dpacked, None, self.S, self.D, HD)
        self._unpack("pos_kernel")


ATTENTION_KEYS = ("key_dim", "n_head", "kernel_size", "ff_kernel_size", "ff_multiplier", "ff_factor0", "ff_factor1")


def check_attention_config(cfg: dict, stage: bool = False, D=None, dropout: bool = False) -> None:
    """the mandatory keys and the ValueErrors of reference modules.py:513-551 (`depth` is the stage's, modules.py:174); what has no kernel here
    is refused, not ignored"""
    who = f"attention_{'stage' if stage else 'block'}"
    for key in ATTENTION_KEYS + (("depth",) if stage else ()):
        if key not in cfg:
            raise ValueError(f"{who}: missing {key!r}")
    _check_activation(cfg, "swish")
    if _dropout_rate(cfg, who, dropout) > 0 and not bool(cfg.get("abs_pos_encoding", False)):
        raise ValueError(f"{who}: dropout_rate > 0 (absent: the reference's {DROPOUT_DEFAULT}) with abs_pos_encoding False: the relative-position "
                         "kernels (seld_relattn_*) cannot drop their probabilities yet — their backward is four differently laid-out kernels; "
                         "set abs_pos_encoding True or dropout_rate 0")
    f0, f1, fk, fm = float(cfg["ff_factor0"]), float(cfg["ff_factor1"]), int(cfg["ff_kernel_size"]), float(cfg["ff_multiplier"])
    if f0 < 0 or f1 < 0:
        raise ValueError("ff_factor0, ff_factor1 >= 0 must hold")
    if f0 == 0 and f1 == 0:
        if fk > 0:
            raise ValueError("if FF modules are not used, ff_kernel must be set to 0")
        if fm > 0:
            raise ValueError("if FF modules are not used, ff_multiplier must be set to 0")
    _check_pos_encoding(cfg, who, D, relative=not bool(cfg.get("abs_pos_encoding", False)))
    if fk < 0 or fm < 0 or ((f0 > 0 or f1 > 0) and (fk < 1 or (D is not None and int(fm * int(D)) < 1))):
        raise ValueError(f"{who}: a FF module takes ff_kernel_size >= 1 and int(ff_multiplier * d_model) >= 1")
    if int(cfg["n_head"]) < 1 or not 0 <= int(cfg["kernel_size"]) <= 64 or (stage and int(cfg["depth"]) < 1):
        raise ValueError(f"{who}: n_head, depth >= 1 and 0 <= kernel_size <= 64")
    _check_key_dim(cfg["key_dim"])


class _FFModule:
    """attention_block's FF module (modules.py:559-572, 619-632): x + factor Conv1D(D, k)(act(Conv1D(int(ff_multiplier D), k)(x))), then
    LayerNormalization unless layer_norm_in_front — whose own LayerNormalization is dead: the first Conv1D reads x (modules.py:564, 624)."""

    def __init__(self, rt: _Rt, name: str, lname, B: int, S: int, D: int, F: int, k: int, act: int, factor: float, drop: _Drop, sites):
        self.rt, self.S, self.factor, self.drop = rt, S, float(factor), drop
        R = B * S
        self.ffn = _FeedForward(rt, Conv1D(rt, f"{name}a", B, S, D, F, k), Conv1D(rt, f"{name}b", B, S, F, D, k), R, act, self.factor, None, drop, sites)
        self.ln = LayerNorm(rt, lname, R, D) if lname else None
        self.y, self.dx = rt.empty(R, D), rt.empty(R, D)

    def forward(self, x, B, training):
        rt, R = self.rt, B * self.S
        h = self.ffn.hidden(x, R)
        y = self.y[:R]
        y.copy_(x)
        self.drop.add(self.ffn.sites[1], y, self.ffn.second.forward(h, R), self.factor)
        return self.ln.forward(y, None, R, training) if self.ln else y

    def backward(self, dy, B):
        rt, R = self.rt, B * self.S
        dz = self.ln.backward(dy, R) if self.ln else dy
        dx = self.dx[:R]
        self.ffn.backward(dz, dx, R)
        rt.axpy(dx, dz)
        return dx


class AttentionBlock:
    """reference modules.attention_block (modules.py:511-635) on [B, S, D].  In training with dropout_rate > 0 (abs_pos_encoding only) the
    Dropouts draw (_Drop: behind each FF module's activation and output, on the attention probabilities, behind the attention and behind the
    depthwise tail); written without them (lnf = layer_norm_in_front):
      x = FF0(x)                                                   (ff_factor0 > 0)
      a = x; x += table (abs_pos_encoding: AFTER a is taken, so the attention never sees it)
      x = x + MHA(LN?(a))        MultiHeadAttention_ (abs_pos_encoding) or RelPositionMultiHeadAttention with the table;  x = LN(x) unless lnf
      c = GLU(Conv1D(2D, 1)(LN?(x)))                              (use_glu; LN? = with lnf)
      x = x + Conv1D(D, 1)(swish(BN(depthwise Conv1D(k)(c))))     (kernel_size > 0; with lnf and no GLU one LN in front of the depthwise
                                                                   convolution); x = LN(x) unless lnf.  kernel_size = 0: x = c, nothing else
      x = FF1(x)                                                   (ff_factor1 > 0)"""

    def __init__(self, rt: _Rt, cfg: dict, S: int, D: int, prefix: str, B: int):
        check_attention_config(cfg, D=D, dropout=rt.dropout)
        self.rt, self.S, self.D, self.B = rt, int(S), int(D), B
        S, D, p = self.S, self.D, prefix
        R = B * S
        act = ACT[cfg.get("activation", "swish")]
        F, fk = int(cfg["ff_multiplier"] * D), int(cfg["ff_kernel_size"])
        self.lnf, self.glu, self.k = bool(cfg.get("layer_norm_in_front", False)), bool(cfg.get("use_glu", False)), int(cfg["kernel_size"])
        self.abs = bool(cfg.get("abs_pos_encoding", False))
        lnf = self.lnf
        H, dk, ub = int(cfg["n_head"]), int(cfg["key_dim"]), bool(cfg.get("use_bias", False))
        f0, f1 = float(cfg["ff_factor0"]), float(cfg["ff_factor1"])
        self.drop = _Drop(rt, _dropout_rate(cfg, "attention_block", rt.dropout))
        self.ff0 = _FFModule(rt, f"{p}.ff0", None if lnf else f"{p}.ln0", B, S, D, F, fk, act, f0, self.drop, (0, 1)) if f0 > 0 else None
        self.ln1 = LayerNorm(rt, f"{p}.ln1", R, D) if lnf else None
        if self.abs:
            self.mha = MultiHeadAttentionRef(rt, f"{p}.mha", B, S, D, H, dk, ub, self.drop, 2)
        else:
            self.mha = RelPositionMultiHeadAttention(rt, f"{p}.mha", B, S, D, H, dk, ub)
        if not lnf:
            self.ln1 = LayerNorm(rt, f"{p}.ln1", R, D)
        self.ln2 = self.pw0 = self.tail = self.gate = None
        if self.glu:
            if lnf:
                self.ln2 = LayerNorm(rt, f"{p}.ln2", R, D)
            self.pw0 = Conv1D(rt, f"{p}.pw0", B, S, D, 2 * D, 1)
            if self.k == 0:
                self.gate = GLU(rt, R, D)
        if self.k > 0:
            if lnf and not self.glu:
                self.ln2 = LayerNorm(rt, f"{p}.ln2", R, D)
            self.tail = _ConvTail(rt, p, B, S, D, self.k, glu=self.glu)
            if not lnf:
                self.ln2 = LayerNorm(rt, f"{p}.ln2", R, D)
        self.ff1 = _FFModule(rt, f"{p}.ff1", None if lnf else f"{p}.ln3", B, S, D, F, fk, act, f1, self.drop, (5, 6)) if f1 > 0 else None
        self.enc = None
        if self.abs and cfg.get("pos_encoding", "basic") == "basic":
            self.enc = torch.as_tensor(basic_pos_encoding(S, D)).to(rt.dev)
        e = rt.empty
        self.xr, self.xb, self.xc = e(R, D), e(R, D), e(R, D)
        self.du, self.dn, self.dxb, self.dxa = e(R, 2 * D), e(R, D), e(R, D), e(R, D)
        self.dd = e(R, D) if self.drop.rate > 0 else None      # a gradient behind a Dropout
        self.out_dim, self.out_shape = D, (S, D)

    def forward(self, x, B, training):
        """x [B*S, D] (or any contiguous view of it) -> [B*S, D]"""
        rt = self.rt
        R, D = B * self.S, self.D
        x = x.reshape(R, D)
        drop = self.drop
        drop.begin(training)
        if self.ff0:
            x = self.ff0.forward(x, B, training)
        attn = self.ln1.forward(x, None, R, training) if self.lnf else x
        res = x
        if self.enc is not None:
            res = self.xr[:R]
            res.copy_(x)
            rt.ck(rt.lib.seld_pos_add(rt.p(res), rt.p(self.enc), B, self.S, D, rt.st()))
        attn = self.mha.forward(attn, B, training)
        if self.lnf:
            xb = self.xb[:R]
            xb.copy_(res)
            drop.add(3, xb, attn)
        else:
            xb = self.ln1.forward(drop.apply(3, attn, attn) if drop.on else attn, res, R, training)
        c = xb
        if self.glu:
            c = self.pw0.forward(self.ln2.forward(c, None, R, training) if self.lnf else c, R)
            if self.k == 0:
                c = self.gate.forward(c, R)
        if self.k > 0:
            if self.lnf and not self.glu:
                c = self.ln2.forward(c, None, R, training)
            pw = self.tail.forward(c, B, training)
            if self.lnf:
                xc = self.xc[:R]
                xc.copy_(xb)
                drop.add(4, xc, pw)
            else:
                xc = self.ln2.forward(drop.apply(4, pw, pw) if drop.on else pw, xb, R, training)
        else:
            xc = c
        return self.ff1.forward(xc, B, training) if self.ff1 else xc

    def backward(self, dy, B):
        """dy [B*S, D]: the output's gradient -> the input's gradient [B*S, D] (a buffer of this block)"""
        rt = self.rt
        R, D = B * self.S, self.D
        d = dy.reshape(R, D)
        if self.ff1:
            d = self.ff1.backward(d, B)
        dxb, dn = self.dxb[:R], self.dn[:R]
        du = self.du[:R] if self.glu else self.du.view(-1)[:R * D].view(R, D)
        if self.k > 0:
            dz = d if self.lnf else self.ln2.backward(d, R)               # gradient of xb + pw
            dxb.copy_(dz)
            self.tail.backward(self.drop.apply(4, dz, self.dd[:R]) if self.drop.on else dz, du, B)
            if self.glu:
                self.pw0.backward(du, dn, R)
                rt.axpy(dxb, self.ln2.backward(dn, R) if self.lnf else dn)
            else:
                rt.axpy(dxb, self.ln2.backward(du, R) if self.lnf else du)
        elif self.glu:
            self.gate.backward(d, du, R)
            self.pw0.backward(du, dn, R)
            dxb.copy_(self.ln2.backward(dn, R) if self.lnf else dn)
        else:
            dxb.copy_(d)
        dz = dxb if self.lnf else self.ln1.backward(dxb, R)               # gradient of attn + x (the table is a constant)
        dxa = self.dxa[:R]
        dxa.copy_(dz)
        self.mha.backward(self.drop.apply(3, dz, self.dd[:R]) if self.drop.on else dz, dn, B)
        rt.axpy(dxa, self.ln1.backward(dn, R) if self.lnf else dn)
        return self.ff0.backward(dxa, B) if self.ff0 else dxa


RNN_MERGE = ("mul", "concat", "ave", "sum")      # what tf.keras.layers.Bidirectional merges into ONE tensor


def _recurrent_rate(cfg: dict, who: str) -> float:
    """dropout_rate of a recurrent kind whose owner accepted the library's draws, as the fp32 seld_dropout compares with (absent or None: the
    reference's 0, modules.py:306, 329); 0 <= rate < 1"""
    r = float(np.float32(cfg.get("dropout_rate", 0.0) or 0.0))
    if not 0.0 <= r < 1.0:      # NaN fails both comparisons
        raise ValueError(f"{who}: dropout_rate {cfg.get('dropout_rate')!r}: 0 <= dropout_rate < 1")
    return r


GRU_MIN_UNITS, GRU_MAX_UNITS = 1, 256      # seld_rnn_gruw_*


def _is_gru_width(u) -> bool:
    return isinstance(u, (int, np.integer)) and not isinstance(u, bool) and GRU_MIN_UNITS <= int(u) <= GRU_MAX_UNITS


def _check_widths_and_rate(cfg: dict, who: str, widths, any_units: bool, dropout: bool, texts) -> None:
    """The rules check_rnn_config and check_gru_config share, on the layers' `widths` (None: `units` has the wrong form): every width is 128 —
    with any_units an integer in 1..256; the recurrences under dropout (the DROP forms) exist at 128 only; dropout_rate is a rate where the
    owner accepted the library's draws (`dropout`) and 0 elsewhere.  texts: the caller's own words — its refusal of a width with any_units
    and without, how the DROP refusal names the widths, its refusal of a rate without `dropout`"""
    bad_any_width, bad_width, at, no_draws = texts
    rate = float(cfg.get("dropout_rate", 0.0) or 0.0)
    if any_units:
        if widths is None or not all(_is_gru_width(u) for u in widths):
            raise ValueError(bad_any_width)
        if rate != 0.0 and any(int(u) != 128 for u in widths):
            raise ValueError(f"{who}: dropout_rate {cfg.get('dropout_rate')!r} at {at}: the recurrences under dropout / recurrent_dropout (the "
                             "DROP forms) are 128-unit kernels; at another width dropout_rate must be 0")
    elif widths is None or any(int(u) != 128 for u in widths):
        raise ValueError(bad_width)
    if dropout:
        _recurrent_rate(cfg, who)
    elif rate != 0.0:
        raise ValueError(no_draws)


def check_rnn_config(cfg: dict, stage: bool = False, dropout: bool = False, any_units: bool = False) -> None:
    """reference modules.RNN_block / RNN_stage (modules.py:64-83, 322-347): the mandatory keys; what has no kernel here is refused, not ignored.
    dropout: the owner accepted the library's draws for the cells' input and state masks (_Recurrent), and dropout_rate may be any rate in
    [0, 1); without it the rate must be 0.  any_units: a GRU may have any integer width in 1..256 (seld_rnn_gruw_*; the LSTM kernels and
    the DROP forms stay 128-unit kernels)"""
    who = f"RNN_{'stage' if stage else 'block'}"
    for key in ("units",) + (("depth",) if stage else ()):
        if key not in cfg:
            raise ValueError(f"{who}: missing {key!r}")
    u = cfg["units"]
    _check_widths_and_rate(cfg, who, None if isinstance(u, (list, tuple)) else [u], any_units and cfg.get("rnn_type", "GRU") == "GRU", dropout, (
        f"{who}: units {u!r}: a GRU width is an integer in {GRU_MIN_UNITS}..{GRU_MAX_UNITS}",
        f"{who}: units {u!r}: the recurrence kernels are built for 128 units", f"{u} units",
        f"{who}: dropout / recurrent_dropout inside the recurrence kernels (per-clip input and state masks) are not implemented on "
        "the composed path, whose Dropout (seld_dropout, seld_attn_drop_*) covers the attention kinds only: dropout_rate must be 0"))
    if stage and int(cfg["depth"]) < 1:
        raise ValueError(f"{who}: depth >= 1")
    if bool(cfg.get("bidirectional", True)) and cfg.get("merge_mode", "mul") not in RNN_MERGE:
        # None makes Bidirectional return a LIST (the reference's graph breaks on it); 'avg' (the reference's comment) is rejected by Keras itself
        raise ValueError(f"{who}: merge_mode {cfg.get('merge_mode')!r}: one of {RNN_MERGE}")


class _Recurrent:
    """The recurrent blocks' one forward and one backward on [B*S, D] with u units (128; a GRU on a runtime with any_units: 1..256) and gate
    width G (GRU, reset_after=True: 3u, LSTM: 4u).  Per direction `name` of `names`: the variables kernel (D, G), recurrent_kernel (u, G),
    bias (GRU (2, 3u): input row | recurrent row; LSTM (4u,)), the input projections gx, the states h and sv, the pre-activation gradients
    dgx (GRU: and dgh, behind the reset gate); the input's gradient din.  A subclass says WHICH block this is — `lstm`, `bi`, `mode`,
    `fusable`, the buffers `c`, `dh`, `out` — and the path is

        forward    projection: gx = x kernel + input bias, per direction   ->  recurrence (_recurrence)  ->  merge (seld_rnn_merge_fwd; bi)
        backward   merge (seld_rnn_merge_bwd; one direction: dy as given)  ->  recurrence  ->  weight gradients and din (_weight_grads)

    with the recurrence one of (every pair of entries takes ..., B, S, u, stream):

        cell  dropout on  u      fused   entries                    saved for the backward (sv; LSTM: and c)
        GRU   no          128    yes     seld_m_gru_fwd / _bwd      in training; recurrence and the 'mul' merge are one operator
        GRU   no          128    no      seld_rnn_gru_fwd / _bwd    in training
        GRU   no          other  -       seld_rnn_gruw_fwd / _bwd   in training
        GRU   yes         128    -       seld_rnn_gru_drop_*        always; the forward stores the masked states hm as well
        LSTM  no          128    -       seld_rnn_lstm_fwd / _bwd   in training
        LSTM  yes         128    -       seld_rnn_lstm_drop_*       always

    Dropout on = Keras dropout / recurrent_dropout (`rate` > 0 and training; reference modules.py:312-315, 338-340 pass dropout_rate as
    both): every cell — each direction — owns an input mask im [B, D] and a state mask rm [B, u] of 0 | 1 / (1 - rate), drawn once per training
    forward and constant over the sequence: seld_dropout on ones, sites (_Drop) 0 / 1 = the forward direction's input / state mask, 2 / 3 =
    the backward direction's.  A direction then projects its own xm = x * im (seld_rnn_mask_rows) and rm rides in the recurrence; backward,
    the weight gradients read xm and the masked state sequence hm = h * rm, and din = the sum over the directions of (dgx kernel^T) * im."""
    fusable = False      # at 128 units without dropout, the recurrences and the 'mul' merge are the fused seld_m_gru_fwd / _bwd

    def __init__(self, rt: _Rt, names, S: int, D: int, G: int, B: int, rate: float = 0.0, units: int = 128):
        """units: the width u (a GRU on a runtime with any_units: 1..256, G = 3u; otherwise 128; under dropout 128)"""
        self.rt, self.names, self.S, self.D, self.G, self.B, self.u = rt, names, int(S), int(D), G, B, int(units)
        u = self.u
        assert G == (4 * u if self.lstm else 3 * u) and (u == 128 or (not self.lstm and rate == 0.0))
        for n in names:
            rt.var(f"{n}.kernel", (self.D, G)); rt.var(f"{n}.recurrent_kernel", (u, G)); rt.var(f"{n}.bias", (G,) if self.lstm else (2, G))
            rt.recurrent.append((B * self.S, self.D, u, G))
        R, nd = B * self.S, len(names)
        e = rt.empty
        self.gx, self.h, self.sv = [e(R, G) for _ in range(nd)], [e(R, u) for _ in range(nd)], [e(R, 4 * u) for _ in range(nd)]
        self.dgx = [e(R, G) for _ in range(nd)]
        self.dgh = [e(R, G) for _ in range(nd)] if not self.lstm else self.dgx      # LSTM: no reset gate, one pre-activation gradient
        self.din = e(R, self.D)
        self.drop = _Drop(rt, rate)
        if rate > 0.0:
            if self.D % 4:
                raise ValueError(f"recurrent dropout on an input width of {self.D}: the mask kernel (seld_rnn_mask_rows) moves float4, D % 4 == 0")
            self.ones = torch.ones(B * max(self.D, u), dtype=torch.float32, device=rt.dev)
            self.im, self.rm = [e(B, self.D) for _ in range(nd)], [e(B, u) for _ in range(nd)]
            self.xm, self.hm = [e(R, self.D) for _ in range(nd)], [e(R, u) for _ in range(nd)]
            self.dxm = e(R, self.D)

    def _pair(self, ts, none=False):
        """the (forward, backward) pointer pair of a per-direction buffer list; one direction: (pointer, NULL)"""
        p = self.rt.p
        return (None, None) if none else (p(ts[0]), p(ts[1]) if len(self.names) == 2 else None)

    def _mask_rows(self, src, mask, dst, R, F, accumulate=0):
        rt = self.rt
        rt.ck(rt.lib.seld_rnn_mask_rows(rt.p(src), rt.p(mask), rt.p(dst), R, self.S, F, int(accumulate), rt.st()))

    def _fused(self):
        return self.fusable and self.u == 128 and not self.drop.on

    def _recurrence(self, training=True):
        """The recurrence of the current forward (the class's table) -> (stem, forward pointers, backward pointers): the calls are
        `stem`_fwd(*forward pointers, B, S, u, stream) and `stem`_bwd(*output gradients, *backward pointers, B, S, u, stream)"""
        rt, P, drop = self.rt, self._pair, self.drop.on
        gx, h, U = P(self.gx), P(self.h), P([rt.w(f"{n}.recurrent_kernel") for n in self.names])
        sv = P(self.sv, none=not (training or drop))      # inference saves nothing; the DROP forms always save
        rm = P(self.rm) if drop else ()
        if self.lstm:
            return ("seld_rnn_lstm_drop" if drop else "seld_rnn_lstm", gx + U + rm + h + P(self.c, none=not (training or drop)) + sv,
                    P(self.c) + sv + U + rm + P(self.dgx))
        brec = P([rt.w(f"{n}.bias")[self.G:] for n in self.names])
        dg = P(self.dgx) + P(self.dgh)
        if drop:
            return "seld_rnn_gru_drop", gx + U + brec + rm + h + P(self.hm) + sv, P(self.hm) + sv + U + rm + dg
        if self._fused():
            return "seld_m_gru", gx + U + brec + h + sv + (rt.p(self.out),), h + sv + U + dg
        return "seld_rnn_gru" if self.u == 128 else "seld_rnn_gruw", gx + U + brec + h + sv, h + sv + U + dg

    def forward(self, x, B, training):
        """x [B*S, D] (or any contiguous view of it) -> [B*S, out_dim]"""
        rt, R = self.rt, B * self.S
        self.drop.begin(training)
        self.x = x = x.reshape(R, self.D)
        for d, n in enumerate(self.names):      # gx = x kernel + the input bias, per direction; under dropout from the direction's own xm = x * im
            if self.drop.on:
                self.drop.apply(2 * d, self.ones[:B * self.D], self.im[d][:B])
                self.drop.apply(2 * d + 1, self.ones[:B * self.u], self.rm[d][:B])
                self._mask_rows(x, self.im[d], self.xm[d], R, self.D)
            rt.gemm(self.xm[d] if self.drop.on else x, rt.w(f"{n}.kernel"), rt.w(f"{n}.bias")[:self.G], self.gx[d], R, self.G, self.D)
        stem, pointers, _ = self._recurrence(training)
        rt.ck(getattr(rt.lib, stem + "_fwd")(*pointers, B, self.S, self.u, rt.st()))
        if not self.bi:
            return self.h[0][:R]
        if not self._fused():
            rt.ck(rt.lib.seld_rnn_merge_fwd(rt.p(self.h[0]), rt.p(self.h[1]), rt.p(self.out), R, self.u, self.mode, rt.st()))
        return self.out[:R]

    def backward(self, dy, B):
        """dy [B*S, out_dim]: the output's gradient (after a training forward) -> the input's gradient [B*S, D] (a buffer of this block)"""
        rt, R = self.rt, B * self.S
        dy = dy.reshape(R, self.out_dim)
        if self._fused():      # the kernel forms the 'mul' merge's gradient itself
            dh = (rt.p(dy),)
        elif self.bi:
            rt.ck(rt.lib.seld_rnn_merge_bwd(rt.p(dy), rt.p(self.h[0]), rt.p(self.h[1]), rt.p(self.dh[0]), rt.p(self.dh[1]), R, self.u, self.mode,
                                            rt.st()))
            dh = self._pair(self.dh)
        else:
            self._dy = dy.contiguous()      # kept: the kernel reads it after this call returns
            dh = (rt.p(self._dy), None)
        stem, _, pointers = self._recurrence()
        rt.ck(getattr(rt.lib, stem + "_bwd")(*dh, *pointers, B, self.S, self.u, rt.st()))
        return self._weight_grads(R)

    def _weight_grads(self, R):
        """dgx, dgh -> every variable's gradient and the input's [R, D]; under dropout from the masked xm and hm, and through the input mask"""
        rt, drop = self.rt, self.drop.on
        for d, n in enumerate(self.names):
            gb = rt.g(f"{n}.bias")
            if drop and self.lstm:      # the GRU kernel stored its masked state sequence
                self._mask_rows(self.h[d], self.rm[d], self.hm[d], R, self.u)
            rt.gemm_tn(self.xm[d] if drop else self.x, self.dgx[d], rt.g(f"{n}.kernel"), gb[:self.G], R, self.D, self.G)
            # recurrent kernel: h_prev^T dgh — the forward direction saw h[t-1], the backward direction h[t+1]
            rt.gemm_tn(self.hm[d] if drop else self.h[d], self.dgh[d], rt.g(f"{n}.recurrent_kernel"), None if self.lstm else gb[self.G:], R, self.u,
                       self.G, seq=self.S, shift=-1 if d == 0 else 1)
            if drop:
                rt.gemm(self.dgx[d], rt.w(f"{n}.kernel"), None, self.dxm, R, self.D, self.G, transb=1)
                self._mask_rows(self.dxm, self.im[d], self.din, R, self.D, accumulate=d)
            else:
                rt.gemm(self.dgx[d], rt.w(f"{n}.kernel"), None, self.din, R, self.D, self.G, transb=1, accumulate=d)
        return self.din[:R]


class RNNBlock(_Recurrent):
    """reference modules.RNN_block (modules.py:322-347) on [B*S, D]: rnn_type 'GRU' -> GRU(128, reset_after=True), ANYTHING else -> LSTM(128)
    (modules.py:334-337), return_sequences=True; bidirectional -> Bidirectional(merge_mode), whose variables are the forward layer's, then the
    backward layer's (`{prefix}.fwd.*`, `{prefix}.bwd.*`; one direction: `{prefix}.*`).  With bidirectional=False merge_mode is ignored.
    GRU: kernel (D, 384), recurrent_kernel (128, 384), bias (2, 384);  LSTM: kernel (D, 512), recurrent_kernel (128, 512), bias (512,).
    The configuration picks the row of _Recurrent's table (`lstm`, the width, dropout_rate > 0 on a runtime whose owner accepted the library's
    draws) and the merge (`bi`, `mode`); this class owns what only some of those need: the LSTM's cell states c, the directions' output
    gradients dh and the merged output."""

    def __init__(self, rt: _Rt, cfg: dict, S: int, D: int, prefix: str, B: int):
        check_rnn_config(cfg, dropout=rt.dropout, any_units=rt.any_units)
        self.prefix = prefix
        self.lstm = cfg.get("rnn_type", "GRU") != "GRU"
        self.bi = bool(cfg.get("bidirectional", True))
        self.mode = _lib.SELD_MERGE[cfg.get("merge_mode", "mul")] if self.bi else None
        u = int(cfg["units"])
        super().__init__(rt, [f"{prefix}.fwd", f"{prefix}.bwd"] if self.bi else [prefix], S, D, 4 * u if self.lstm else 3 * u, B,
                         _recurrent_rate(cfg, "RNN_block") if rt.dropout else 0.0, u)
        self.out_dim = 2 * u if self.bi and cfg.get("merge_mode", "mul") == "concat" else u
        R, nd = B * self.S, len(self.names)
        e = rt.empty
        self.c = [e(R, u) for _ in range(nd)] if self.lstm else None
        self.dh = [e(R, u) for _ in range(nd)] if self.bi else None
        self.out = e(R, self.out_dim) if self.bi else None
        self.out_shape = (self.S, self.out_dim)


def check_gru_config(cfg: dict, stage: bool = False, dropout: bool = False, any_units: bool = False) -> None:
    """reference modules.bidirectional_GRU_block (modules.py:302-319): one layer per entry of `units`.  dropout, any_units: as
    check_rnn_config's"""
    u = cfg["units"]
    listed = isinstance(u, (list, tuple))
    _check_widths_and_rate(cfg, "bidirectional_GRU_block", u if listed or not any_units else None, any_units, dropout, (
        f"bidirectional_GRU_block: units {u!r}: a list of integers in {GRU_MIN_UNITS}..{GRU_MAX_UNITS}, one per layer",
        "the recurrence kernels are built for 128 units", f"units {list(u)!r}" if listed else "",
        "bidirectional_GRU_block: GRU dropout / recurrent_dropout masks exist on the fused path only (models.SeldNet), not among "
        "the composed path's Dropout operators: dropout_rate must be 0"))


class BidirectionalGRUBlock(_Recurrent):
    """One layer of reference modules.bidirectional_GRU_block (modules.py:302-319) on [B*S, D]: Bidirectional(GRU(units[layer],
    return_sequences=True), merge_mode='mul') on _Recurrent's path.  What differs from an RNN_block with the same cell: at 128 units, when no
    dropout is drawn, the recurrences and the 'mul' merge are ONE operator (seld_m_gru_fwd / _bwd: `fusable`), so the per-direction output
    gradients dh exist only for the other forms (dropout_rate > 0, or another width)."""
    lstm, bi, mode, fusable = False, True, _lib.SELD_MERGE["mul"], True
    PER_LAYER_UNITS = True      # Stage passes `layer`, the block's index in the stage: its width is cfg['units'][layer]

    def __init__(self, rt: _Rt, cfg: dict, S: int, D: int, prefix: str, B: int, layer: int = 0):
        check_gru_config(cfg, dropout=rt.dropout, any_units=rt.any_units)
        u = int(cfg["units"][layer])
        super().__init__(rt, [f"{prefix}.fwd", f"{prefix}.bwd"], S, D, 3 * u, B,
                         _recurrent_rate(cfg, "bidirectional_GRU_block") if rt.dropout else 0.0, u)
        self.out = rt.empty(B * self.S, u)
        self.dh = [rt.empty(B * self.S, u) for _ in (0, 1)] if self.drop.rate > 0.0 or u != 128 else None
        self.out_dim, self.out_shape = u, (self.S, u)


class _SqueezeExcite:
    """mother_block's squeeze-and-excitation tail (reference modules.py:281-296) on [B, H, W, C]: x * sigmoid(Conv2D(C, 1)(act(Conv2D(sf, 1)(
    mean over H, W of x)))) — on one pixel the two 1x1 convolutions are Linear layers with Keras' kernels (1, 1, C, sf) and (1, 1, sf, C)."""

    def __init__(self, rt: _Rt, prefix: str, shape, sf: int, act: int, B: int):
        self.rt, self.shape, self.act = rt, tuple(shape), act
        Cc = self.shape[2]
        self.se0 = Linear(rt, f"{prefix}.se0", B, Cc, sf, (1, 1, Cc, sf))
        self.se1 = Linear(rt, f"{prefix}.se1", B, sf, Cc, (1, 1, sf, Cc))
        e = rt.empty
        self.m, self.s1, self.s2, self.y = e(B, Cc), e(B, sf), e(B, Cc), e(B, *self.shape)
        self.ds2, self.da2, self.ds1, self.da1, self.dm, self.din = e(B, Cc), e(B, Cc), e(B, sf), e(B, sf), e(B, Cc), e(B, *self.shape)

    def forward(self, x, B):
        rt = self.rt
        Hh, Ww, Cc = self.shape
        self.x = x
        rt.ck(rt.lib.seld_m_mean_hw(rt.p(x), rt.p(self.m), B, Hh * Ww, Cc, rt.st()))
        rt.act(self.se0.forward(self.m, B), self.s1[:B], self.act)
        rt.act(self.se1.forward(self.s1, B), self.s2[:B], ACT["sigmoid"])
        rt.ck(rt.lib.seld_m_scale_hw(rt.p(x), rt.p(self.s2), rt.p(self.y), B, Hh * Ww, Cc, rt.st()))
        return self.y[:B]

    def backward(self, dy, B):
        """dy: the output's gradient -> the input's (a buffer of this layer)"""
        rt = self.rt
        Hh, Ww, Cc = self.shape
        rt.ck(rt.lib.seld_m_scale_hw_bwd_ds(rt.p(self.x), rt.p(dy), rt.p(self.ds2), B, Hh * Ww, Cc, rt.st()))
        rt.act_bwd(self.se1.z[:B], self.ds2[:B], self.da2[:B], ACT["sigmoid"])
        self.se1.backward(self.da2, self.ds1, B)
        rt.act_bwd(self.se0.z[:B], self.ds1[:B], self.da1[:B], self.act)
        self.se0.backward(self.da1, self.dm, B)
        rt.ck(rt.lib.seld_m_scale_hw_bwd_dx(rt.p(dy), rt.p(self.s2), rt.p(self.dm), rt.p(self.din), B, Hh * Ww, Cc, 0, rt.st()))
        return self.din[:B]


class MotherBlock:
    """reference modules.mother_block (modules.py:184-298)."""

    def __init__(self, rt: _Rt, cfg: dict, in_shape, prefix: str, B: int):
        check_mother_config(cfg)
        self.rt, self.cfg, self.B = rt, cfg, B
        f = [int(cfg[f"filters{i}"]) for i in range(3)]
        k = [int(cfg[f"kernel_size{i}"]) for i in range(3)]
        conn = [list(cfg["connect0"]), list(cfg["connect1"]), list(cfg["connect2"])]
        strides = safe_tuple(cfg.get("strides", (1, 1)))
        self.act = ACT[cfg.get("activation", "relu")]
        self.f, self.conn, self.strides = f, conn, strides
        shapes = [tuple(in_shape)]
        self.layers = []      # per layer: dict(kind='conv'|'alias'|'cat'|'dead', ...)
        dead = dead_layers(cfg) + (False,)
        for L in range(3):
            src = shapes[-1]
            n_in = L + 1      # outputs[0..L] exist
            lay = {"L": L}
            if dead[L]:
                # the layer's output reaches nothing: Keras' functional model does not contain it: no variables, no computation
                lay.update(kind="dead")
                out = src if f[L] == 0 else (-(-src[0] // (strides[0] if L == 1 else 1)), -(-src[1] // (strides[1] if L == 1 else 1)), f[L])
            elif f[L] > 0:
                s = strides if L == 1 else (1, 1)
                main = _ConvBN(rt, f"{prefix}.c{L}", f"{prefix}.bn{L}", src, f[L], k[L], s, B)
                out = main.out_shape
                skips = []
                for i in range(n_in):
                    if conn[L][i] != 1:
                        continue
                    if shapes[i] != out:
                        ps = (1, 1) if (L == 2 and i == 2) or L == 0 else strides
                        skips.append((i, _ConvBN(rt, f"{prefix}.p{L}_{i}", f"{prefix}.pbn{L}_{i}", shapes[i], f[L], 1, ps, B)))
                    else:
                        skips.append((i, None))
                lay.update(kind="conv", main=main, skips=skips, pre=rt.empty(B, *out), y=rt.empty(B, *out), dpre=rt.empty(B, *out))
            elif L == 0:
                out = src
                lay.update(kind="alias")
            else:
                parts = []
                for i in range(n_in):
                    if conn[L][i] != 1:
                        continue
                    s = shapes[i]
                    cv = None
                    if L == 2 and conn[2][-1] == 1 and strides != (1, 1) and i < 2:
                        cv = Conv2D(rt, f"{prefix}.s2_{i}", s, s[2], 1, strides, B)      # connect with strided outputs
                        s = cv.out_shape
                    parts.append((i, cv, s))
                if len({p[2][:2] for p in parts}) != 1:
                    raise ValueError("mother_block: the concatenated tensors differ in their spatial extents")
                out = (parts[0][2][0], parts[0][2][1], sum(p[2][2] for p in parts))
                lay.update(kind="cat", parts=parts, y=rt.empty(B, *out), tmp=rt.empty(B, *out))
            lay["out"] = out
            self.layers.append(lay)
            if L < 2:
                shapes.append(out)
        self.shapes = shapes
        self.out_shape = self.layers[2]["out"]
        sq = float(cfg.get("squeeze_ratio", 0))
        self.se = None
        if sq > 0:
            self.se = _SqueezeExcite(rt, prefix, self.out_shape, int(sq * self.out_shape[2]), ACT[cfg.get("se_activation", "relu")], B)
        # gradients w.r.t. outputs[0..2] (outputs[0] = the block input) are accumulated here during backward
        self.gout = [rt.empty(B, *s) for s in shapes]

    # ---------------------------------------------------------------- forward
    def forward(self, x, B, training):
        rt = self.rt
        outputs = [x]
        res = None
        for lay in self.layers:
            L = lay["L"]
            if lay["kind"] == "dead":
                y = None
            elif lay["kind"] == "alias":
                y = outputs[-1]
            elif lay["kind"] == "conv":
                pre = lay["pre"][:B]
                lay["main"].forward(outputs[-1], pre, B, training, accumulate=0)
                for i, proj in lay["skips"]:
                    if proj is None:
                        rt.axpy(pre, outputs[i])
                    else:
                        proj.forward(outputs[i], pre, B, training, accumulate=1)
                y = lay["y"][:B]
                rt.act(pre, y, self.act)
            else:
                y = lay["y"][:B]
                Cd, off = lay["out"][2], 0
                rows = B * lay["out"][0] * lay["out"][1]
                for i, cv, s in lay["parts"]:
                    src = outputs[i] if cv is None else cv.forward(outputs[i], B)
                    rt.ck(rt.lib.seld_m_copy_channels(rt.p(src), rt.p(y), rows, s[2], Cd, off, 0, rt.st()))
                    off += s[2]
            if L < 2:
                outputs.append(y)
            else:
                res = y
        self.outputs = outputs
        return res if self.se is None else self.se.forward(res, B)

    # ---------------------------------------------------------------- backward
    def backward(self, dy, dx, B, need_dx=True):
        """dy: gradient w.r.t. the block output; dx (= the caller's buffer for the block input's gradient, overwritten) or None"""
        rt = self.rt
        if self.se is not None:
            dy = self.se.backward(dy, B)
        # gradient slots of outputs[0..2]; outputs[1] may alias outputs[0] (first layer skipped): then they share one slot
        alias0 = self.layers[0]["kind"] == "alias"
        slots = [self.gout[0][:B], self.gout[0][:B] if alias0 else self.gout[1][:B], self.gout[2][:B]]
        written = [False, False, False]

        def slot_of(i):
            return 0 if (i == 1 and alias0) else i

        def add_to(i, src):
            j = slot_of(i)
            if written[j]:
                rt.axpy(slots[j], src)
            else:
                slots[j].copy_(src)       # device-to-device copy on the current stream
                written[j] = True

        for lay in reversed(self.layers):
            L = lay["L"]
            d_out = dy if L == 2 else (slots[slot_of(L + 1)] if written[slot_of(L + 1)] else None)
            if lay["kind"] in ("alias", "dead"):
                continue          # outputs[1] IS outputs[0]: its gradient already sits in slot 0 / a dead layer has neither variables nor a gradient
            if d_out is None:
                raise RuntimeError("mother_block: a layer's output reaches nothing (the configuration checks should have refused it)")
            src_i = L             # the layer's main input is outputs[L]
            if lay["kind"] == "conv":
                dpre = lay["dpre"][:B]
                rt.act_bwd(lay["pre"][:B], d_out, dpre, self.act)
                j = slot_of(src_i)
                lay["main"].backward(dpre, slots[j], B, accumulate=written[j])
                written[j] = True
                for i, proj in lay["skips"]:
                    if proj is None:
                        add_to(i, dpre)
                    else:
                        jj = slot_of(i)
                        proj.backward(dpre, slots[jj], B, accumulate=written[jj])
                        written[jj] = True
            else:
                Cd, off = lay["out"][2], 0
                rows = B * lay["out"][0] * lay["out"][1]
                for i, cv, s in lay["parts"]:
                    if cv is None:
                        jj = slot_of(i)
                        if not written[jj]:
                            slots[jj].zero_()
                            written[jj] = True
                        rt.ck(rt.lib.seld_m_copy_channels(rt.p(slots[jj]), rt.p(d_out), rows, s[2], Cd, off, 1, rt.st()))
                    else:
                        piece = lay["tmp"][:B].reshape(-1)[:rows * s[2]].view(B, s[0], s[1], s[2])
                        piece.zero_()
                        rt.ck(rt.lib.seld_m_copy_channels(rt.p(piece), rt.p(d_out), rows, s[2], Cd, off, 1, rt.st()))
                        jj = slot_of(i)
                        cv.backward(piece, slots[jj], B, accumulate=written[jj])
                        written[jj] = True
                    off += s[2]
        if dx is not None:
            dx.copy_(slots[0])
        return slots[0]


COMPOSED_SECOND = ("bidirectional_GRU_block", "transformer_encoder_block", "transformer_encoder_stage")
CONFORMER_SECOND = ("conformer_encoder_block", "conformer_encoder_stage")      # SECOND as well: COMPOSED_SECOND + CONFORMER_SECOND
ATTENTION_SECOND = ("attention_block", "attention_stage")                          # SECOND as well, routed as CONFORMER_SECOND is
RNN_SECOND = ("RNN_block", "RNN_stage")                                            # SECOND as well; the heads read the stage's out_dim


# SECOND kind -> (block class, its config check, the variables' prefix, a *_stage of cfg['depth'] blocks?, does the check take the width D?)
SECOND_KINDS = {
    "bidirectional_GRU_block": (BidirectionalGRUBlock, check_gru_config, "gru", False, False),      # one layer per entry of `units`
    "transformer_encoder_block": (TransformerEncoderBlock, check_transformer_config, "tf", False, False),
    "transformer_encoder_stage": (TransformerEncoderBlock, check_transformer_config, "tf", True, False),
    "conformer_encoder_block": (ConformerEncoderBlock, check_conformer_config, "cf", False, True),
    "conformer_encoder_stage": (ConformerEncoderBlock, check_conformer_config, "cf", True, True),
    "attention_block": (AttentionBlock, check_attention_config, "at", False, True),
    "attention_stage": (AttentionBlock, check_attention_config, "at", True, True),
    "RNN_block": (RNNBlock, check_rnn_config, "rnn", False, False),
    "RNN_stage": (RNNBlock, check_rnn_config, "rnn", True, False),
}
assert tuple(SECOND_KINDS) == COMPOSED_SECOND + CONFORMER_SECOND + ATTENTION_SECOND + RNN_SECOND


DROPOUT_KINDS = COMPOSED_SECOND + CONFORMER_SECOND + ATTENTION_SECOND + RNN_SECOND      # the SECOND kinds whose Dropouts can draw (_Drop): all


def _check_second(kind: str, cfg: dict, D=None, dropout: bool = False, any_units: bool = False, any_key_dim: bool = False) -> None:
    _, check, _, stage, with_d = SECOND_KINDS[kind]
    kw = {"dropout": True} if dropout and kind in DROPOUT_KINDS else {}
    if any_units and check in (check_gru_config, check_rnn_config):
        kw["any_units"] = True
    if any_key_dim and check in (check_transformer_config, check_conformer_config):
        kw["any_key_dim"] = True
    check(cfg, stage, D, **kw) if with_d else check(cfg, stage, **kw)


def _build_second(kind: str, rt, cfg: dict, S: int, D: int, B: int, prefix=None, dropout: bool = False, first_block: int = 0) -> Stage:
    """the SECOND stage `kind` on [B*S, D] (rt None: on a runtime of its own on the current device); the configuration errors, those that
    need the width among them (pos_encoding 'basic' on an odd one, the FF width), are raised first, without a device.  dropout: the caller
    accepts the library's draws (_dropout_rate); a given rt carries its owner's choice"""
    block, _, pre, stage, _ = SECOND_KINDS[kind]
    dropout = bool(dropout) if rt is None else rt.dropout
    _check_second(kind, cfg, D, dropout, rt is not None and rt.any_units, rt is not None and rt.any_key_dim)
    own = rt is None
    rt = rt or _Rt(torch.device("cuda", torch.cuda.current_device()))
    rt.dropout = dropout
    depth = int(cfg["depth"]) if stage else len(cfg["units"]) if block is BidirectionalGRUBlock else 1
    st = Stage(rt, block, cfg, S, D, prefix or pre, B, depth, first_block)
    st.model = own
    return st


def check_dense_config(cfg: dict, dropout: bool = False) -> float:
    """reference modules.simple_dense_block (modules.py:350-376) as a body block -> its dropout_rate as the fp32 the kernels compare with.
    dropout: the owner wires the block's Dropout layers (seld_dropout behind each activation: models.vad_architecture) and the rate may be
    any in [0, 1); without it the rate must be 0, as before"""
    if "units" not in cfg or not isinstance(cfg["units"], (list, tuple)):
        raise ValueError("simple_dense_block: `units` is a list, one entry per layer")
    if any(int(u) < 1 for u in cfg["units"]) or int(cfg.get("kernel_size", 1)) < 1:
        raise ValueError("simple_dense_block: units and kernel_size >= 1")
    _check_activation(cfg, None, "dense_activation")
    if dropout:
        rate = float(np.float32(cfg.get("dropout_rate", 0) or 0))
        if not 0.0 <= rate < 1.0:
            raise ValueError(f"simple_dense_block: dropout_rate {cfg.get('dropout_rate')!r}: 0 <= dropout_rate < 1")
        return rate
    if float(cfg.get("dropout_rate", 0) or 0) != 0.0:
        raise ValueError("simple_dense_block: dropout_rate must be 0 — its Dropout layers are wired on the fused path only (models.SeldNet), as for "
                         "the composed heads; the composed path's Dropout covers the attention kinds")
    return 0.0


class DenseBlock:
    """reference modules.simple_dense_block (modules.py:350-376) as a body block on [B*S, D]: one Conv1D(units, kernel_size, 'same') +
    dense_activation per entry of `units` (variables `{prefix}.dense{j}`), out_dim = the last width; `units` = []: the identity (which is
    also what identity_block is, modules.py:639-642).  dropout (models.vad_architecture): a dropout_rate above 0 puts seld_dropout behind
    each layer's activation (modules.py:372-373), site j = the layer, on the block's own streams DROP_STREAM0 + 32 * first_block + j (_Drop);
    training only.  flat: the input is the reference's 2-D tensor (S = 1), where the block builds Dense — kernel (D, u), kernel_size unused."""

    def __init__(self, rt: _Rt, cfg: dict, S: int, D: int, prefix: str, B: int, dropout: bool = False, first_block: int = 0, flat: bool = False):
        rate = check_dense_config(cfg, dropout)
        self.rt, self.S, self.D = rt, int(S), int(D)
        self.act = ACT[cfg.get("dense_activation", None)]
        self.drop = _Drop(rt, rate)
        self.drop.base = DROP_STREAM0 + 32 * int(first_block)
        k, R = int(cfg.get("kernel_size", 1)), B * self.S
        if flat and self.S != 1:
            raise ValueError("simple_dense_block: a 2-D input has no time axis (S = 1)")
        self.layers = []      # (layer, its activation y, the gradient of its pre-activation, the gradient of its input, of y behind the Dropout)
        for j, u in enumerate(int(u) for u in cfg["units"]):
            lin = Dense(rt, f"{prefix}.dense{j}", R, D, u) if flat else Conv1D(rt, f"{prefix}.dense{j}", B, self.S, D, u, k)
            self.layers.append((lin, rt.empty(R, u), rt.empty(R, u), rt.empty(R, D), rt.empty(R, u) if rate > 0.0 else None))
            D = u
        self.out_dim, self.out_shape = int(D), (self.S, int(D))

    def forward(self, x, B, training):
        R = B * self.S
        x = x.reshape(R, self.D)
        self.drop.begin(training)
        for j, (lin, y, _, _, _) in enumerate(self.layers):
            self.rt.act(lin.forward(x, R), y[:R], self.act)
            if self.drop.on:
                self.drop.apply(j, y[:R], y[:R])
            x = y[:R]
        return x

    def backward(self, dy, B):
        R = B * self.S
        for j, (lin, _, dpre, dx, dd) in reversed(list(enumerate(self.layers))):
            if self.drop.on:
                dy = self.drop.apply(j, dy, dd[:R])
            self.rt.act_bwd(lin.z[:R], dy, dpre[:R], self.act)
            lin.backward(dpre[:R], dx[:R], R)
            dy = dx[:R]
        return dy


class Head:
    """reference modules.simple_dense_block (modules.py:350-376) with kernel_size 1 on [rows, Cin]: a Conv1D(u, 1) (kernel (1, Cin, u)) +
    `hact` per entry of `units`, then Dense(n_out) (kernel (Cin, n_out)) + `act`.  backward starts from `dpre`, the gradient of the output
    layer's pre-activation, which the loss kernel writes."""

    def __init__(self, rt: _Rt, name: str, rows: int, Cin: int, units, hact: int, n_out: int, act: int):
        self.rt, self.hact, self.act = rt, hact, act
        self.hidden = []      # (layer, its activation y, the gradients of its pre-activation and of y)
        for j, u in enumerate(int(u) for u in units):
            self.hidden.append((Linear(rt, f"{name}.dense{j}", rows, Cin, u, (1, Cin, u)), rt.empty(rows, u), rt.empty(rows, u), rt.empty(rows, u)))
            Cin = u
        self.out = Linear(rt, f"{name}.out", rows, Cin, n_out)
        self.dpre = rt.empty(rows, n_out)

    def forward(self, x, y, rows):
        """x [rows, Cin] -> y [rows, n_out] (the caller's)"""
        for lin, a, _, _ in self.hidden:
            self.rt.act(lin.forward(x, rows), a[:rows], self.hact)
            x = a
        self.rt.act(self.out.forward(x, rows), y, self.act)

    def backward(self, dx, rows, accumulate):
        """dpre -> every variable's gradient; dx (+)= the input's gradient"""
        lin, dz = self.out, self.dpre
        for hid, _, dpre, da in reversed(self.hidden):
            lin.backward(dz, da, rows)
            self.rt.act_bwd(hid.z[:rows], da[:rows], dpre[:rows], self.hact)
            lin, dz = hid, dpre
        lin.backward(dz, dx, rows, accumulate)


def v2_unit_shape(shape):
    """utils.unitwise_norm (utils.py:71-83) as [rows][cols] with one clip unit per column, launch_agc's mapping: rank <= 1 one unit; rank 2 and
    3 the norm over axis 0 alone (a head-major (H, D, dk) kernel is H rows of D * dk units: the reference as written); rank 4 over the
    first three axes.  A higher rank raises, as the reference does."""
    sh = tuple(int(v) for v in shape)
    if len(sh) <= 1:
        return int(np.prod(sh)), 1
    if len(sh) in (2, 3):
        return sh[0], int(np.prod(sh[1:]))
    if len(sh) == 4:
        return int(np.prod(sh[:3])), sh[3]
    raise ValueError(f"Got a parameter with shape not in [1, 2, 4]! {sh}")


class ComposedSeldNet:
    """models.seldnet(input_shape, model_config) (reference models.py:18-32) composed from module operators: FIRST = mother_block |
    mother_stage, SECOND = bidirectional_GRU_block (units 128: the recurrence kernels) | transformer_encoder_block | transformer_encoder_stage |
    conformer_encoder_block | conformer_encoder_stage | attention_block | attention_stage (d_model = F * C of the FIRST stage's output) |
    RNN_block | RNN_stage (GRU or LSTM, units 128; the heads read 128 features, or 256 behind merge_mode 'concat'),
    SED / DOA = simple_dense_block (kernel_size 1).  The conformer and attention stages' BatchNormalization statistics join `state_variables`
    behind the FIRST block's."""

    def __init__(self, input_shape, model_config: dict, device=None):
        from .models import canonical_config
        if not torch.cuda.is_available():
            raise RuntimeError("seld_amd needs a HIP device: there is no CPU fallback")
        cfg = canonical_config(model_config)
        seconds = tuple(SECOND_KINDS)
        if cfg.get("SECOND") not in seconds or cfg.get("SED") != "simple_dense_block" or cfg.get("DOA") != "simple_dense_block":
            raise ValueError(f"composed models: SECOND in {seconds}, SED / DOA = simple_dense_block")
        self._dev = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
        B, T, Fq, Ch = (int(v) for v in input_shape)
        self.input_shape = (B, T, Fq, Ch)
        self.n_classes = int(cfg.get("n_classes", 14))
        rt = self.rt = _Rt(self._dev)
        rt.dropout = True      # a model trains on the library's Dropout draws (dropout_seed / dropout_step below), as the fused models do
        self.lib = rt.lib
        fa = cfg["FIRST_ARGS"]
        if cfg["FIRST"] == "mother_stage":
            cfgs, c = [], copy.deepcopy(fa)
            for _ in range(int(fa["depth"])):
                cfgs.append(copy.deepcopy(c))
                c["strides"] = (1, 1)       # modules.py:41
        elif cfg["FIRST"] == "mother_block":
            cfgs = [copy.deepcopy(fa)]
        else:
            raise ValueError(f"composed models: FIRST = mother_block | mother_stage, not {cfg['FIRST']!r}")
        shape = (T, Fq, Ch)
        self.blocks = []
        for d, c in enumerate(cfgs):
            blk = MotherBlock(rt, c, shape, f"mb{d}", B)
            self.blocks.append(blk)
            shape = blk.out_shape
        self.S = shape[0]
        self.second = _build_second(cfg["SECOND"], rt, cfg["SECOND_ARGS"], self.S, shape[1] * shape[2], B)      # d_model = F * C (force_1d_inputs)
        fin = self.second.out_dim
        self.heads = []
        for head, key, n_out, act in (("sed", "SED_ARGS", self.n_classes, "sigmoid"), ("doa", "DOA_ARGS", 3 * self.n_classes, "tanh")):
            ha = cfg[key]
            if int(ha.get("kernel_size", 1)) != 1 or float(ha.get("dropout_rate", 0)) != 0:
                raise ValueError("composed heads: kernel_size 1 and no dropout — the heads' Dropout (simple_dense_block) is wired on the fused path only; "
                                 "the composed path's Dropout covers the attention SECOND kinds")
            hact = ha.get("dense_activation", None)
            if hact not in ACT:
                raise ValueError(f"dense_activation {hact!r}")
            self.heads.append(Head(rt, head, B * self.S, fin, ha.get("units", []), ACT[hact], n_out, ACT[act]))
        rt.finalize()
        self.variables, self.state_variables = rt.variables, rt.state_variables
        self.n_params, self.n_state = rt.n_params, rt.n_state
        self.dfeat = rt.empty(B * self.S, fin)
        self.loss_scratch = rt.empty(int(rt.lib.seld_m_losses_scratch(B * self.S)))
        self.dfirst = rt.empty(B, *shape)
        self.adam_step = 0
        self._marks = None          # profile(True): [(group name, torch event)] of the current step (bench.py's mother_stage record)
        self._init_weights()

    # ---------------------------------------------------------------- weights
    def _init_weights(self, seed: int = 0):
        rng = np.random.default_rng(seed)
        w = np.zeros(self.n_params, np.float32)
        for n, off, sh in self.variables:
            k = int(np.prod(sh))
            if n.endswith("recurrent_kernel") and sh[1] == 512:      # LSTM: Keras' Orthogonal over the whole [128, 512]
                q, r = np.linalg.qr(rng.standard_normal((512, 128)))
                w[off:off + k] = (q * np.sign(np.diag(r))).T.reshape(-1)
            elif n.endswith("recurrent_kernel"):      # GRU [u, 3u]: an orthogonal [u, u] per gate
                w[off:off + k] = np.concatenate([np.linalg.qr(rng.standard_normal((sh[0], sh[0])))[0] for _ in range(3)], axis=1).reshape(-1)
            elif n.startswith("rnn") and n.endswith("bias") and sh == (512,):
                w[off + 128:off + 256] = 1.0                          # LSTM unit_forget_bias: the forget slice of i | f | c | o
            elif n.endswith(("kernel", "pos_bias_u", "pos_bias_v")):      # the two biases take the kernel initializer (layers.py:343-356)
                fan_in = int(np.prod(sh[:-1])); fan_out = int(sh[-1]) * (int(np.prod(sh[:-2])) if len(sh) > 2 else 1)
                lim = math.sqrt(6.0 / (fan_in + fan_out))
                w[off:off + k] = rng.uniform(-lim, lim, k)
            elif n.endswith("gamma"):
                w[off:off + k] = 1.0
        s = np.zeros(max(self.n_state, 1), np.float32)
        for n, off, sh in self.state_variables:
            if n.endswith("moving_variance"):
                s[off:off + int(np.prod(sh))] = 1.0
        self.set_weights(w, s[:self.n_state])

    def get_weights(self):
        return self.rt.params[:self.n_params].cpu().numpy().copy(), self.rt.state[:self.n_state].cpu().numpy().copy()

    def set_weights(self, w, state=None):
        self.rt.params[:self.n_params].copy_(torch.as_tensor(np.asarray(w, np.float32)))
        if state is not None and self.n_state:
            self.rt.state[:self.n_state].copy_(torch.as_tensor(np.asarray(state, np.float32)))

    def get_grads(self):
        return self.rt.grads[:self.n_params].cpu().numpy().copy()

    def summary(self) -> str:
        lines = [f"ComposedSeldNet input {self.input_shape} -> sed [B,{self.S},{self.n_classes}], doa [B,{self.S},{3 * self.n_classes}]"]
        lines += [f"  {n:32s} {str(sh):20s} {int(np.prod(sh)):8d}" for n, _, sh in self.variables]
        lines.append(f"Trainable params: {self.n_params}; non-trainable: {self.n_state}")
        text = "\n".join(lines)
        print(text)
        return text

    def save_weights(self, path: str) -> None:
        w, s = self.get_weights()
        d = {n: w[o:o + int(np.prod(sh))].reshape(sh) for n, o, sh in self.variables}
        d.update({n: s[o:o + int(np.prod(sh))].reshape(sh) for n, o, sh in self.state_variables})
        np.savez(path, **d)

    def load_weights(self, path: str) -> None:
        z = np.load(path)
        w, s = self.get_weights()
        for n, o, sh in self.variables:
            w[o:o + int(np.prod(sh))] = np.asarray(z[n], np.float32).reshape(-1)
        for n, o, sh in self.state_variables:
            s[o:o + int(np.prod(sh))] = np.asarray(z[n], np.float32).reshape(-1)
        self.set_weights(w, s)

    def close(self) -> None:
        """frees what the model holds outside torch's allocator: the v2 optimizer plan"""
        plan, self._v2_plan = getattr(self, "_v2_plan", None), None
        if plan is not None:
            self.rt.lib.seld_v2_plan_destroy(plan)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---------------------------------------------------------------- measurement aid
    def profile(self, on: bool) -> None:
        """on: every step records a HIP event (torch's current stream) at its phase boundaries; `phase_ms()` gives the phases' durations"""
        self._marks = [] if on else None

    def _mark(self, name: str) -> None:
        if self._marks is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record(torch.cuda.current_stream(self._dev))
            self._marks.append((name, e))

    def phase_ms(self) -> dict:
        """{phase: ms summed over the recorded steps}; call after a synchronize.  A phase lasts from the previous mark to its own."""
        out: Dict[str, float] = {}
        marks, self._marks = self._marks or [], []
        for (_, e0), (n1, e1) in zip(marks[:-1], marks[1:]):
            if n1 != "step_start":
                out[n1] = out.get(n1, 0.0) + e0.elapsed_time(e1)
        return out

    def conv_macs(self) -> int:
        """multiply-adds of the FIRST stage's convolutions (main, projection and strided-concatenation convs) per clip, forward"""
        tot = 0
        for blk in self.blocks:
            for lay in blk.layers:
                convs = []
                if lay["kind"] == "conv":
                    convs = [lay["main"].conv] + [p.conv for _, p in lay["skips"] if p is not None]
                elif lay["kind"] == "cat":
                    convs = [cv for _, cv, _ in lay["parts"] if cv is not None]
                tot += sum(cv.Ho * cv.Wo * cv.K * cv.N for cv in convs)
        return tot

    # ---------------------------------------------------------------- forward / backward
    def _prep(self, x):
        if not (isinstance(x, torch.Tensor) and x.is_cuda):
            x = torch.as_tensor(np.asarray(x), dtype=torch.float32).to(self._dev)
        x = x.to(torch.float32).contiguous()
        Bm, T, Fq, Ch = self.input_shape
        # any batch 1 <= B <= the one the buffers were sized for, as SeldNet._prep: train.main builds the model for the largest of the train /
        # val / test batch sizes and every loader ends on a ragged batch (drop_remainder=False)
        if tuple(x.shape[1:]) != (T, Fq, Ch) or not 1 <= x.shape[0] <= Bm:
            raise ValueError(f"x shape {tuple(x.shape)}: a composed model built for {self.input_shape} runs batches of 1..{Bm} clips of {(T, Fq, Ch)}")
        return x

    # the Dropout draws (attention SECOND kinds with dropout_rate > 0): masks are a function of (dropout_seed, step, layer, element); every
    # training forward takes the next step.  Settable, as the fused models' options of the same names.
    @property
    def dropout_seed(self) -> int:
        return self.rt.dropout_seed

    @dropout_seed.setter
    def dropout_seed(self, v: int) -> None:
        self.rt.dropout_seed = int(v) & 0xffffffffffffffff

    @property
    def dropout_step(self) -> int:
        """the step counter the NEXT training forward draws its masks with"""
        return self.rt.dropout_step

    @dropout_step.setter
    def dropout_step(self, v: int) -> None:
        self.rt.dropout_step = int(v) & 0xffffffff

    def _forward(self, x, training: bool):
        rt = self.rt
        B = x.shape[0]
        if training:
            rt.next_draws()
        h = x
        for blk in self.blocks:
            h = blk.forward(h, B, training)
        self._mark("first_fwd")
        R = B * self.S
        feat = self.second.forward(h.reshape(R, -1), B, training)      # layers.force_1d_inputs (layers.py:41-47): feature = f * C + c
        sed = rt.empty(B, self.S, self.n_classes)
        doa = rt.empty(B, self.S, 3 * self.n_classes)
        for head, out in zip(self.heads, (sed, doa)):
            head.forward(feat, out.view(R, -1), R)
        self._mark("gru_heads_fwd")
        return sed, doa

    def __call__(self, x, training: bool = False):
        x = self._prep(x)
        sed, doa = self._forward(x, bool(training))
        return [sed, doa]

    def _backward(self, B):
        """from the heads' pre-activation gradients (Head.dpre, written by seld_m_losses) to every variable's gradient"""
        R = B * self.S
        for i, head in enumerate(self.heads):
            head.backward(self.dfeat, R, accumulate=int(i > 0))      # the second head adds to the first one's
        dout = self.second.backward(self.dfeat[:R], B)
        self._mark("heads_gru_bwd")
        dy = dout[:R].view(B, *self.blocks[-1].out_shape)
        for bi in range(len(self.blocks) - 1, -1, -1):
            dy = self.blocks[bi].backward(dy, None, B)
        self._mark("first_bwd")

    def _labels(self, y, B):
        ys = torch.as_tensor(y[0], dtype=torch.float32, device=self._dev).contiguous()
        yd = torch.as_tensor(y[1], dtype=torch.float32, device=self._dev).contiguous()
        if tuple(ys.shape) != (B, self.S, self.n_classes) or tuple(yd.shape) != (B, self.S, 3 * self.n_classes):
            raise ValueError(f"label shapes {tuple(ys.shape)}, {tuple(yd.shape)} do not match the model output")
        return ys, yd

    def _losses(self, sed, doa, ys, yd, cfg, want_grads):
        from . import losses
        rt = self.rt
        B = sed.shape[0]
        sloss = torch.empty((), dtype=torch.float32, device=self._dev)
        dloss = torch.empty((B, self.S) if cfg.doa_loss != 1 else (), dtype=torch.float32, device=self._dev)
        rt.ck(rt.lib.seld_m_losses(rt.p(sed), rt.p(doa), rt.p(ys), rt.p(yd), C.byref(cfg), rt.p(sloss), rt.p(dloss),
                                   rt.p(self.heads[0].dpre) if want_grads else None, rt.p(self.heads[1].dpre) if want_grads else None,
                                   rt.p(self.loss_scratch), B, self.S, self.n_classes, rt.st()))
        return sloss, dloss

    def train_step(self, x, y, cfg, optimizer, agc: bool = False):
        """train.trainstep (train.py:22-36) -> ([sed, doa], sloss, dloss)"""
        if agc:
            raise ValueError("adaptive gradient clipping is not wired for composed models")
        rt = self.rt
        x = self._prep(x)
        B = x.shape[0]
        ys, yd = self._labels(y, B)
        self._mark("step_start")
        sed, doa = self._forward(x, True)
        sloss, dloss = self._losses(sed, doa, ys, yd, cfg, True)
        self._mark("losses")
        self._backward(B)
        self.adam_step += 1
        rt.ck(rt.lib.seld_m_adam(rt.p(rt.params), rt.p(rt.grads), rt.p(rt.adam_m), rt.p(rt.adam_v), self.n_params, optimizer.learning_rate,
                                 optimizer.beta_1, optimizer.beta_2, optimizer.epsilon, self.adam_step, rt.st()))
        self._mark("adam")
        return [sed, doa], sloss, dloss

    def test_step(self, x, y, cfg):
        x = self._prep(x)
        ys, yd = self._labels(y, x.shape[0])
        sed, doa = self._forward(x, False)
        sloss, dloss = self._losses(sed, doa, ys, yd, cfg, False)
        return [sed, doa], sloss, dloss

    # ---------------------------------------------------------------- the trainv2 recipe (trainv2.py:23-56, swa.py)
    def set_regularized(self, flags) -> None:
        """one flag per trainable variable: the variables the L2 kernel regulariser covers (trainv2.apply_kernel_regularizer sets them);
        the optimizer plan is rebuilt at the next step when they changed"""
        flags = [int(bool(f)) for f in flags]
        if len(flags) != len(self.variables):
            raise ValueError("set_regularized: one flag per trainable variable")
        if flags != getattr(self, "_v2_flags", None):
            self.close()
            self._v2_flags = flags

    def _v2_get_plan(self):
        if getattr(self, "_v2_plan", None) is None:
            nv = len(self.variables)
            flags = getattr(self, "_v2_flags", None) or [0] * nv
            rc = [v2_unit_shape(sh) for _, _, sh in self.variables]
            plan = C.c_void_p()
            self.rt.ck(self.rt.lib.seld_v2_plan_create(self.n_params, nv, (C.c_int64 * nv)(*[off for _, off, _ in self.variables]),
                                                         (C.c_int32 * nv)(*[r for r, _ in rc]), (C.c_int32 * nv)(*[c for _, c in rc]),
                                                         (C.c_int32 * nv)(*flags), C.byref(plan)))
            self._v2_plan = plan
        return self._v2_plan

    def _v2_fwd_bwd(self, x, y, v2cfg):
        """forward, the weighted losses (seld_v2_losses writes the heads' dpre), backward -> ([sed, doa], sloss, dloss); rt.grads holds
        every variable's raw gradient"""
        rt = self.rt
        x = self._prep(x)
        B = x.shape[0]
        ys, yd = self._labels(y, B)
        if self.n_classes > _lib.V2_MAX_CLASSES:
            raise ValueError(f"the v2 losses take at most {_lib.V2_MAX_CLASSES} classes")
        self._mark("step_start")
        sed, doa = self._forward(x, True)
        sloss = torch.empty((), dtype=torch.float32, device=self._dev)
        dloss = torch.empty((), dtype=torch.float32, device=self._dev)
        rt.ck(rt.lib.seld_v2_losses(rt.p(sed), rt.p(doa), rt.p(ys), rt.p(yd), C.byref(v2cfg), rt.p(sloss), rt.p(dloss), rt.p(self.heads[0].dpre),
                                      rt.p(self.heads[1].dpre), rt.p(self.loss_scratch), B, self.S, self.n_classes, rt.st()))
        self._mark("losses")
        self._backward(B)
        return [sed, doa], sloss, dloss

    def _v2_opt(self, optimizer, l2: float = 0.0, clip_factor: float = 0.01):
        """regulariser + AGC + AdaBelief on the flat buffers, two launches; the AdaBelief slots are the Adam slots, as on the fused path"""
        rt = self.rt
        plan = self._v2_get_plan()
        self.adam_step += 1
        rt.ck(rt.lib.seld_v2_opt(plan, rt.p(rt.params), rt.p(rt.grads), rt.p(rt.adam_m), rt.p(rt.adam_v), optimizer.learning_rate, optimizer.beta_1,
                                   optimizer.beta_2, optimizer.epsilon, float(l2), float(clip_factor), self.adam_step, rt.st()))
        self._mark("v2_opt")

    def train_step_v2(self, x, y, v2cfg, optimizer, l2: float = 0.0, clip_factor: float = 0.01):
        """trainv2.trainstep (trainv2.py:33-56) -> ([sed, doa], sloss, dloss); v2cfg: _lib.V2Cfg; no host synchronisation"""
        if l2 < 0:
            raise ValueError("l2 must be >= 0")
        self._v2_get_plan()      # its one-time allocation and copies come before the step's first launch
        out = self._v2_fwd_bwd(x, y, v2cfg)
        self._v2_opt(optimizer, l2, clip_factor)
        return out

    @property
    def swa_count(self) -> int:
        return getattr(self, "_swa_cnt", 0)

    def swa_update(self) -> None:
        """swa.SWA.update_swa_weights (swa.py:25-32) over the weights and the BatchNormalization statistics; the buffers are allocated at the
        first update"""
        rt = self.rt
        if getattr(self, "_swa_w", None) is None:
            self._swa_w, self._swa_s, self._swa_cnt = rt.empty(max(self.n_params, 1)), rt.empty(max(self.n_state, 1)), 0
        rt.ck(rt.lib.seld_v2_swa(rt.p(self._swa_w), rt.p(rt.params), self.n_params, self._swa_cnt, rt.st()))
        if self.n_state:
            rt.ck(rt.lib.seld_v2_swa(rt.p(self._swa_s), rt.p(rt.state), self.n_state, self._swa_cnt, rt.st()))
        self._swa_cnt += 1

    def swa_apply(self) -> None:
        """swa.SWA.on_train_end: the averages become the model's weights and statistics"""
        if self.swa_count == 0:
            raise ValueError("swa_apply before the first swa_update")
        self.rt.params[:self.n_params].copy_(self._swa_w[:self.n_params])
        if self.n_state:
            self.rt.state[:self.n_state].copy_(self._swa_s[:self.n_state])


CHAIN_4D = ("mother_block", "mother_stage")
# the kinds that take [B, S, D] (each applies layers.force_1d_inputs to a 4-D input: a free reshape in NHWC, D = F * C)
CHAIN_3D = tuple(SECOND_KINDS) + ("bidirectional_GRU_stage", "simple_dense_block", "simple_dense_stage", "identity_block")


def chain_blocks(model_config: dict):
    """models.conv_temporal's block keys in the reference's order (models.py:66-68): the BLOCK* keys that do not end in _ARGS, sorted as
    STRINGS (BLOCK10 comes before BLOCK2)"""
    return sorted(k for k in model_config if k.startswith("BLOCK") and not k.endswith("_ARGS"))


def canonical_kind(kind: str, args: dict):
    """one block of a chain through models.canonical_config's rules: bidirectional_GRU_stage -> bidirectional_GRU_block (depth x [units]),
    simple_dense_stage -> simple_dense_block (depth x [units], dense_activation = args.get('activation'): whatever dense_activation the
    configuration holds is overwritten, reference modules.py:101), identity_block -> simple_dense_block without layers"""
    from .models import canonical_config
    if kind == "bidirectional_GRU_stage":
        c = canonical_config({"SECOND": kind, "SECOND_ARGS": args})
        return c["SECOND"], c["SECOND_ARGS"]
    if kind in ("simple_dense_stage", "identity_block"):
        c = canonical_config({"SED": kind, "SED_ARGS": args})
        return c["SED"], c["SED_ARGS"]
    return kind, copy.deepcopy(args)


class _StageHead:
    """A head of models.conv_temporal (models.py:73-76): any 3-D kind applied to the chain's output, then Dense(n_out) + `act`.  `dpre`: the
    gradient of the output layer's pre-activation, which the loss kernel writes (the interface of Head)."""

    def __init__(self, rt: _Rt, name: str, body, rows: int, n_out: int, act: int):
        self.rt, self.body, self.act = rt, body, act
        self.out = Linear(rt, f"{name}_out", rows, body.out_dim, n_out)
        self.dpre = rt.empty(rows, n_out)
        self.dbody = rt.empty(rows, body.out_dim)

    def forward(self, x, y, B, rows, training):
        self.rt.act(self.out.forward(self.body.forward(x, B, training), rows), y, self.act)

    def backward(self, B, rows):
        """dpre -> every variable's gradient; returns the gradient of the head's input (a buffer of the head's)"""
        self.out.backward(self.dpre, self.dbody, rows)
        return self.body.backward(self.dbody[:rows], B)


class ConvTemporalNet(ComposedSeldNet):
    """models.conv_temporal(input_shape, model_config) (reference models.py:54-78) composed from module operators:

      stem    StemConv2D(filters, first_kernel_size) -> BatchNormalization -> relu -> MaxPool2D(first_pool_size, 'same')
      blocks  the BLOCK* keys in string order (chain_blocks): mother_block / mother_stage while the tensor is 4-D; the first 3-D kind
              (CHAIN_3D) flattens it to [B, S, F * C], and a 4-D kind behind a 3-D one is a ValueError
      heads   SED and DOA: any 3-D kind on the chain's output, then Dense(n_classes, sigmoid) / Dense(3 n_classes, tanh)

    Variables in the reference's creation order: stem.conv, stem.bn, b{i}.*, sed.*, sed_out, doa.*, doa_out; the BatchNormalization
    statistics in `state_variables` in the same order.  Weights I/O, the losses, train_step / test_step, profile and batches of 1 .. B are
    ComposedSeldNet's.  Every stage of the chain draws its Dropout masks from streams of its own (Stage: first_block).  device='meta': the
    plan alone — variables and shapes without a device (nothing can be run).

    search=True (the architecture search, nas_seldnet): what its search spaces draw and the default refuses is built — a GRU kind of any
    width in 1..256 (_Rt.any_units: seld_rnn_gruw_* at widths other than 128), a transformer / conformer encoder kind of any key_dim in
    1..64 (_Rt.any_key_dim: seld_attnw_* at key_dims that are no multiple of 8) and simple_dense_block's Dropout layers on the library's
    draws (DenseBlock dropout=True, as in VadArchNet).  What the default builds, it builds with the same calls: the same bits."""

    DENSE_KW: dict = {}      # what _build_3d passes to a DenseBlock beyond its place in the chain (search / VadArchNet: dropout; VadArchNet: flat)

    def __init__(self, input_shape, model_config: dict, device=None, search: bool = False):
        cfg = copy.deepcopy(model_config)
        meta = device == "meta"
        if not meta and not torch.cuda.is_available():
            ConvTemporalNet(input_shape, cfg, "meta", search)      # the configuration errors first, as the factories raise them without a device
            raise RuntimeError("seld_amd needs a HIP device: there is no CPU fallback")
        self._dev = torch.device("meta") if meta else torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
        B, T, Fq, Ch = (int(v) for v in input_shape)
        self.input_shape = (B, T, Fq, Ch)
        self.n_classes = int(cfg.get("n_classes", 14))
        rt = self.rt = _Rt(self._dev)
        rt.dropout = True
        self.search = bool(search)
        if self.search:
            rt.any_units = True
            rt.any_key_dim = True
            self.DENSE_KW = {"dropout": True}
        self.lib = rt.lib
        # ---- stem (layers.conv2d_bn + MaxPooling2D, models.py:62-64)
        self.stem_conv = StemConv2D(rt, "stem.conv", (T, Fq, Ch), int(cfg.get("filters", 32)), int(cfg.get("first_kernel_size", 7)), B)
        self.stem_bn = BatchNorm(rt, "stem.bn", self.stem_conv.out_shape, B)
        self.stem_pre, self.stem_act = rt.empty(B, *self.stem_conv.out_shape), rt.empty(B, *self.stem_conv.out_shape)
        self.stem_dact, self.stem_dz = rt.empty(B, *self.stem_conv.out_shape), rt.empty(B, *self.stem_conv.out_shape)
        self.pool = MaxPool2D(rt, self.stem_conv.out_shape, cfg.get("first_pool_size", [5, 1]), B, "same")
        shape = self.pool.out_shape
        # ---- the chain
        self.blocks, self.body = [], []      # 4-D blocks (MotherBlock), 3-D blocks (Stage / DenseBlock)
        self.stream_bases = {}                # prefix of a Stage -> its first Dropout stream
        self.n_built = 0
        D = None
        for i, key in enumerate(chain_blocks(cfg)):
            kind, args = cfg[key], cfg.get(f"{key}_ARGS")
            if args is None:
                raise ValueError(f"conv_temporal: {key} has no {key}_ARGS")
            if kind in CHAIN_4D:
                if D is not None:
                    raise ValueError(f"conv_temporal: {key} = {kind!r} takes a 4-D tensor, but a block in front of it has made it 3-D")
                cfgs, c = [], copy.deepcopy(args)
                for _ in range(int(args["depth"]) if kind == "mother_stage" else 1):
                    cfgs.append(copy.deepcopy(c))
                    c["strides"] = (1, 1)       # modules.py:41
                for d, c in enumerate(cfgs):
                    blk = MotherBlock(rt, c, shape, f"b{i}.mb{d}", B)
                    self.blocks.append(blk)
                    shape = blk.out_shape
                    self.n_built += 1
            elif kind in CHAIN_3D:
                if D is None:
                    D = shape[1] * shape[2]      # layers.force_1d_inputs (layers.py:41-47): feature = f * C + c
                blk = self._build_3d(kind, args, shape[0], D, B, f"b{i}")
                self.body.append(blk)
                D = blk.out_dim
            else:
                raise ValueError(f"conv_temporal: {key} = {kind!r}: one of {CHAIN_4D + CHAIN_3D}")
        self.shape4 = shape                   # the tensor behind the last 4-D block
        self.S = shape[0]
        four_d = D is None
        if four_d:
            D = shape[1] * shape[2]
        R = B * self.S
        self.heads = []
        for head, n_out, act in (("sed", self.n_classes, "sigmoid"), ("doa", 3 * self.n_classes, "tanh")):
            kind, args = cfg.get(head.upper()), cfg.get(f"{head.upper()}_ARGS", {})
            if kind not in CHAIN_3D:
                raise ValueError(f"conv_temporal: {head.upper()} = {kind!r}: one of {CHAIN_3D}")
            if four_d and kind == "identity_block":
                raise ValueError(f"conv_temporal: {head.upper()} = identity_block on a 4-D tensor: the reference's Dense would give a 4-D output")
            self.heads.append(_StageHead(rt, head, self._build_3d(kind, args, self.S, D, B, head), R, n_out, ACT[act]))
        rt.finalize()
        self.variables, self.state_variables = rt.variables, rt.state_variables
        self.n_params, self.n_state = rt.n_params, rt.n_state
        self.dfeat = rt.empty(R, D)
        self.loss_scratch = rt.empty(int(rt.lib.seld_m_losses_scratch(R)))
        self.adam_step = 0
        self._marks = None
        if not meta:
            self._init_weights()

    def _build_3d(self, kind: str, args: dict, S: int, D: int, B: int, prefix: str):
        kind, args = canonical_kind(kind, args)
        if kind == "simple_dense_block":
            blk = DenseBlock(self.rt, args, S, D, prefix, B, first_block=self.n_built, **self.DENSE_KW)
            self.n_built += 1
            return blk
        pre = SECOND_KINDS[kind][2]
        st = _build_second(kind, self.rt, args, S, D, B, prefix=f"{prefix}.{pre}", first_block=self.n_built)
        self.stream_bases[f"{prefix}.{pre}"] = DROP_STREAM0 + 32 * self.n_built
        self.n_built += len(st.blocks)
        return st

    def summary(self) -> str:
        return super().summary().replace("ComposedSeldNet", "ConvTemporalNet", 1)

    def complexity(self) -> dict:
        """{'flops', 'params'}: params = n_params; flops = the multiply-adds per clip of the plan's products — as VadArchNet.complexity(), the
        sum over every Linear layer (Dense, Conv1D, Conv2D, the stem, the heads) of (rows / B) K N, plus what the recurrent layers multiply
        outside a Linear, per direction and layer: the input projection S D G and the recurrent product S u G (GRU: G = 3u, LSTM: 4u).  Our
        own count, read off the plan: it is NOT claimed to equal the reference's model_complexity.conv_temporal_complexity (closed forms per
        stage, which also count normalisations and activations)."""
        B = self.input_shape[0]
        flops = sum((rows // B) * K * N for rows, K, N in self.rt.linears)
        flops += sum((rows // B) * (D + u) * G for rows, D, u, G in self.rt.recurrent)
        return {"flops": int(flops), "params": int(self.n_params)}

    def _forward(self, x, training: bool):
        rt = self.rt
        B = x.shape[0]
        if training:
            rt.next_draws()
        z = self.stem_conv.forward(x, B)
        self.stem_bn.forward(z, self.stem_pre[:B], B, training, 0)
        rt.act(self.stem_pre[:B], self.stem_act[:B], ACT["relu"])
        h = self.pool.forward(self.stem_act[:B], B, training)
        for blk in self.blocks:
            h = blk.forward(h, B, training)
        self._mark("first_fwd")
        R = B * self.S
        h = h.reshape(R, -1)
        for blk in self.body:
            h = blk.forward(h, B, training)
        sed = rt.empty(B, self.S, self.n_classes)
        doa = rt.empty(B, self.S, 3 * self.n_classes)
        for head, out in zip(self.heads, (sed, doa)):
            head.forward(h, out.view(R, -1), B, R, training)
        self._mark("gru_heads_fwd")
        return sed, doa

    def _backward(self, B):
        """from the heads' pre-activation gradients (written by seld_m_losses) to every variable's gradient"""
        rt = self.rt
        R = B * self.S
        dy = self.dfeat[:R]
        for i, head in enumerate(self.heads):
            d = head.backward(B, R)
            if i == 0:
                dy.copy_(d.reshape(R, -1))
            else:
                rt.axpy(dy, d)      # the second head's gradient adds to the first one's
        for blk in reversed(self.body):
            dy = blk.backward(dy, B)
        self._mark("heads_gru_bwd")
        dy = dy[:R].reshape(B, *self.shape4)
        for blk in reversed(self.blocks):
            dy = blk.backward(dy, None, B)
        dact = self.pool.backward(dy, B)
        rt.act_bwd(self.stem_pre[:B], dact, self.stem_dact[:B], ACT["relu"])
        self.stem_bn.backward(self.stem_dact[:B], self.stem_dz[:B], B)
        self.stem_conv.backward(self.stem_dz[:B], B)
        self._mark("first_bwd")


DENSE_KINDS = ("simple_dense_block", "simple_dense_stage", "identity_block")      # the 3-D kinds that also take the reference's 2-D tensor


class VadArchNet(ComposedSeldNet):
    """models.vad_architecture(input_shape = (B, Wn, F, C), model_config) (reference models.py:81-102) composed from module operators:

      flatten (default True)   the window becomes [B, Wn F C]: the reference's 2-D tensor, on which simple_dense_block builds Dense (variables
                               (D, u)) and nothing with a time axis or a Conv2D can follow — only DENSE_KINDS; a 4-D kind is a ValueError
      blocks  the BLOCK* keys in string order (chain_blocks): mother_block / mother_stage while the tensor is 4-D; the first 3-D kind
              (CHAIN_3D, built by ConvTemporalNet._build_3d) flattens it to [B, Wn, F C]; a 4-D kind behind a 3-D one is a ValueError.
              simple_dense_block's Dropout layers are wired here (DenseBlock dropout=True)
      head    layers.force_1d_inputs, Dense(last_unit, sigmoid) (variables out.kernel (D, last_unit), out.bias), the trailing axis squeezed
              where last_unit = 1: the prediction is [B, last_unit] (flatten) or [B, Wn', last_unit]
      loss    binary cross-entropy against a label of the prediction's shape (nas_vad.py:172-173)

    fused_head: True — the head runs on seld_vadarch_head_fwd / _bwd (csrc/vadarch.hip; last_unit <= 8), which give the loss, dx, dw and db
    from one read of x; False — Linear + seld_m_act + seld_vad_bce + seld_m_act_bwd; None — FUSED_HEAD where last_unit <= 8 (tools/
    bench_vadarch.py measures one against the other: DESIGN.md section 3x).  Weights I/O, summary, the Dropout counters and batches of
    1 .. B are ComposedSeldNet's; device='meta': the plan alone."""
    FUSED_HEAD = True
    MAX_FUSED_UNITS = 8      # SELD_VADARCH_MAX_U
    _build_3d = ConvTemporalNet._build_3d

    def __init__(self, input_shape, model_config: dict, device=None, fused_head=None):
        cfg = copy.deepcopy(model_config)
        meta = device == "meta"
        if not meta and not torch.cuda.is_available():
            VadArchNet(input_shape, cfg, "meta", fused_head)      # the configuration errors first, without a device
            raise RuntimeError("seld_amd needs a HIP device: there is no CPU fallback")
        self._dev = torch.device("meta") if meta else torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
        if len(input_shape) != 4 or min(int(v) for v in input_shape) < 1:
            raise ValueError(f"vad_architecture: input_shape {tuple(input_shape)!r}: [B, Wn, F, C], all >= 1")
        B, Wn, Fq, Ch = (int(v) for v in input_shape)
        self.input_shape = (B, Wn, Fq, Ch)
        self.flatten, self.last_unit = bool(cfg.get("flatten", True)), int(cfg.get("last_unit", 1))
        if self.last_unit < 1:
            raise ValueError(f"vad_architecture: last_unit {cfg.get('last_unit')!r} must be >= 1")
        if fused_head and self.last_unit > self.MAX_FUSED_UNITS:
            raise ValueError(f"vad_architecture: the fused head takes last_unit <= {self.MAX_FUSED_UNITS}, not {self.last_unit}")
        self.fused = (self.FUSED_HEAD and self.last_unit <= self.MAX_FUSED_UNITS) if fused_head is None else bool(fused_head)
        rt = self.rt = _Rt(self._dev)
        rt.dropout = True
        self.lib = rt.lib
        self.DENSE_KW = {"dropout": True, "flat": self.flatten}
        self.blocks, self.body, self.stream_bases, self.n_built = [], [], {}, 0
        shape = (Wn, Fq, Ch)
        S, D = (1, Wn * Fq * Ch) if self.flatten else (Wn, None)
        for i, key in enumerate(chain_blocks(cfg)):
            kind, args = cfg[key], cfg.get(f"{key}_ARGS")
            if args is None:
                raise ValueError(f"vad_architecture: {key} has no {key}_ARGS")
            if kind in CHAIN_4D:
                if self.flatten:
                    raise ValueError(f"vad_architecture: {key} = {kind!r} takes a 4-D tensor, but flatten has made the input 2-D")
                if D is not None:
                    raise ValueError(f"vad_architecture: {key} = {kind!r} takes a 4-D tensor, but a block in front of it has made it 3-D")
                cfgs, c = [], copy.deepcopy(args)
                for _ in range(int(args["depth"]) if kind == "mother_stage" else 1):
                    cfgs.append(copy.deepcopy(c))
                    c["strides"] = (1, 1)       # modules.py:41
                for d, c in enumerate(cfgs):
                    blk = MotherBlock(rt, c, shape, f"b{i}.mb{d}", B)
                    self.blocks.append(blk)
                    shape = blk.out_shape
                    self.n_built += 1
            elif kind in CHAIN_3D:
                if self.flatten and kind not in DENSE_KINDS:
                    raise ValueError(f"vad_architecture: {key} = {kind!r} needs a time axis, but flatten has made the input 2-D: one of {DENSE_KINDS}")
                if D is None:
                    S, D = shape[0], shape[1] * shape[2]      # layers.force_1d_inputs (layers.py:41-47): feature = f * C + c
                blk = self._build_3d(kind, args, S, D, B, f"b{i}")
                self.body.append(blk)
                D = blk.out_dim
            else:
                raise ValueError(f"vad_architecture: {key} = {kind!r}: one of {CHAIN_4D + CHAIN_3D}")
        self.shape4 = shape
        if D is None:
            S, D = shape[0], shape[1] * shape[2]
        self.S, self.D = int(S), int(D)
        R, U = B * self.S, self.last_unit
        self.on_data = not self.blocks and not any(getattr(b, "layers", True) for b in self.body)      # nothing trainable in front of the head
        if self.fused:      # the kernels read the variables themselves: no Linear, no pre-activation buffer
            rt.var("out.kernel", (self.D, U))
            rt.var("out.bias", (U,))
            rt.linears.append((R, self.D, U))
            self.out = None
        else:
            self.out = Linear(rt, "out", R, self.D, U)
        rt.finalize()
        self.variables, self.state_variables = rt.variables, rt.state_variables
        self.n_params, self.n_state = rt.n_params, rt.n_state
        self.dfeat = None if self.on_data else rt.empty(R, self.D)
        self.d_p, self.dz = (None, None) if self.fused else (rt.empty(R, U), rt.empty(R, U))
        self.loss_scratch = rt.empty(int(rt.lib.seld_vad_bce_scratch(R * U)))
        self.head_scratch = rt.empty(int(rt.lib.seld_vadarch_head_bwd_scratch(R, self.D, U))) if self.fused else None
        self.adam_step = 0
        self._marks = None
        if not meta:
            self._init_weights()

    def output_shape(self, B=None):
        """the prediction's (and the label's) shape for a batch of B windows"""
        B = self.input_shape[0] if B is None else int(B)
        lead = (B,) if self.flatten else (B, self.S)
        return lead if self.last_unit == 1 else lead + (self.last_unit,)

    def summary(self) -> str:
        lines = [f"VadArchNet input {self.input_shape} -> {list(self.output_shape())} ({'fused' if self.fused else 'composed'} head)"]
        lines += [f"  {n:32s} {str(sh):20s} {int(np.prod(sh)):8d}" for n, _, sh in self.variables]
        lines.append(f"Trainable params: {self.n_params}; non-trainable: {self.n_state}")
        text = "\n".join(lines)
        print(text)
        return text

    def complexity(self) -> dict:
        """{'flops', 'params'}: params = n_params; flops = the multiply-adds per window of the plan's dense products, the sum over every
        Linear layer (Dense, Conv1D, Conv2D and projection, the head) of (rows / B) K N.  Our own count, read off the plan: it is NOT claimed
        to equal the reference's model_complexity.vad_architecture_complexity (closed forms per stage, which also count normalisations and
        activations)."""
        B = self.input_shape[0]
        return {"flops": int(sum((rows // B) * K * N for rows, K, N in self.rt.linears)), "params": int(self.n_params)}

    # ---------------------------------------------------------------- forward / backward
    def _forward(self, x, training: bool):
        rt = self.rt
        B = x.shape[0]
        R = B * self.S
        if training:
            rt.next_draws()
        h = x
        for blk in self.blocks:
            h = blk.forward(h, B, training)
        h = h.reshape(R, -1)
        for blk in self.body:
            h = blk.forward(h, B, training)
        return self._head_forward(h, R).view(self.output_shape(B))

    def _head_forward(self, h, R):
        """h [R, D] -> the probabilities [R, last_unit]; h is kept for the backward"""
        rt, U = self.rt, self.last_unit
        self.feat = h
        p = rt.empty(R, U)
        if self.fused:
            rt.ck(rt.lib.seld_vadarch_head_fwd(rt.p(h), rt.p(rt.w("out.kernel")), rt.p(rt.w("out.bias")), rt.p(p), R, self.D, U, rt.st()))
        else:
            rt.act(self.out.forward(h, R), p, ACT["sigmoid"])
        return p

    def __call__(self, x, training: bool = False):
        return self._forward(self._prep(x), bool(training))

    def _label(self, y, B):
        y = torch.as_tensor(y, dtype=torch.float32, device=self._dev).contiguous()
        if tuple(y.shape) != self.output_shape(B):
            raise ValueError(f"label shape {tuple(y.shape)}: the prediction's is {self.output_shape(B)}")
        return y

    def _loss(self, p, y, want_grads: bool):
        """mean binary cross-entropy -> a device scalar; want_grads: the head's variables' gradients and dfeat are written"""
        rt = self.rt
        R, U = p.numel() // self.last_unit, self.last_unit
        loss = torch.empty((), dtype=torch.float32, device=self._dev)
        if self.fused and want_grads:
            rt.ck(rt.lib.seld_vadarch_head_bwd(rt.p(self.feat), rt.p(rt.w("out.kernel")), rt.p(p), rt.p(y), rt.p(loss), rt.p(self.dfeat),
                                               rt.p(rt.g("out.kernel")), rt.p(rt.g("out.bias")), rt.p(self.head_scratch), R, self.D, U, 1.0, rt.st()))
            return loss
        rt.ck(rt.lib.seld_vad_bce(rt.p(p), rt.p(y), rt.p(loss), rt.p(self.d_p) if want_grads else None, rt.p(self.loss_scratch), R * U, 1.0, 0,
                                  rt.st()))
        if want_grads:
            rt.act_bwd(self.out.z[:R], self.d_p[:R], self.dz[:R], ACT["sigmoid"])
            self.out.backward(self.dz, self.dfeat, R)
        return loss

    def _backward(self, B):
        """from dfeat, the gradient of the head's input, to every other variable's gradient"""
        if self.on_data:
            return
        R = B * self.S
        dy = self.dfeat[:R]
        for blk in reversed(self.body):
            dy = blk.backward(dy, B)
        if self.blocks:
            dy = dy[:R].reshape(B, *self.shape4)
            for blk in reversed(self.blocks):
                dy = blk.backward(dy, None, B)

    # ---------------------------------------------------------------- steps
    def train_step(self, x, y, optimizer):
        """one step of model.fit on (x, y of the prediction's shape) -> (prediction, loss).  optimizer: train.Adam (seld_m_adam) or
        trainv2.AdaBelief (seld_v2_opt without regulariser and clipping), as SpectroTemporalVAD takes them; no host synchronisation"""
        from .trainv2 import AdaBelief
        rt = self.rt
        x = self._prep(x)
        B = x.shape[0]
        y = self._label(y, B)
        belief = isinstance(optimizer, AdaBelief)
        if belief:
            self._v2_get_plan()      # its one-time allocation and copies come before the step's first launch
        p = self._forward(x, True)
        loss = self._loss(p, y, True)
        self._backward(B)
        if belief:
            self._v2_opt(optimizer, 0.0, 0.0)
        else:
            self.adam_step += 1
            rt.ck(rt.lib.seld_m_adam(rt.p(rt.params), rt.p(rt.grads), rt.p(rt.adam_m), rt.p(rt.adam_v), self.n_params, optimizer.learning_rate,
                                     optimizer.beta_1, optimizer.beta_2, optimizer.epsilon, self.adam_step, rt.st()))
        return p, loss

    def test_step(self, x, y):
        x = self._prep(x)
        y = self._label(y, x.shape[0])
        p = self._forward(x, False)
        return p, self._loss(p, y, False)

    def train_step_v2(self, *a, **k):
        raise ValueError("the trainv2 recipe (SELD losses) is not this model's: train_step(x, y, optimizer)")


def mother_block(model_config: dict):
    """reference modules.mother_block(model_config) -> a factory `(input_shape, batch) -> MotherBlock`; the configuration errors of
    modules.py:202-222 are raised here, as the reference raises them at construction."""
    check_mother_config(model_config)

    def build(input_shape, rt=None, prefix="mb0"):
        B = int(input_shape[0])
        rt = rt or _Rt(torch.device("cuda", torch.cuda.current_device()))
        return MotherBlock(rt, model_config, tuple(int(v) for v in input_shape[-3:]), prefix, B)
    return build


def _second_factory(kind: str, model_config: dict, dropout: bool = False):
    """dropout (the transformer, conformer and attention kinds): the caller accepts the library's counter-based Dropout draws in place of
    TensorFlow's, and dropout_rate may then be any rate in [0, 1), absent = the reference's 0.1; False: dropout_rate must be present and 0"""
    pre = SECOND_KINDS[kind][2]
    _check_second(kind, model_config, None, dropout)

    def build(input_shape, rt=None, prefix=pre):
        """input_shape [B, S, D] or [B, S, F, C] (layers.force_1d_inputs: D = F * C)"""
        sh = [int(v) for v in input_shape]
        if len(sh) not in (3, 4):
            raise ValueError(f"{kind.replace('_stage', '_block')}: input [B, S, D] or [B, S, F, C]")
        return _build_second(kind, rt, model_config, sh[1], int(np.prod(sh[2:])), sh[0], prefix, dropout)
    return build


def transformer_encoder_block(model_config: dict, dropout: bool = False):
    """reference modules.transformer_encoder_block(model_config) (modules.py:379-407) -> a factory `(input_shape) -> a one-block Stage`
    (forward(x, B, training) / backward(dy, B) on [B*S, D]); configuration errors are raised here, without a device.  dropout: accept the
    library's Dropout draws (_second_factory); without it dropout_rate must be present and 0."""
    return _second_factory("transformer_encoder_block", model_config, dropout)


def transformer_encoder_stage(model_config: dict, dropout: bool = False):
    """reference modules.transformer_encoder_stage(model_config) (modules.py:106-126): `depth` blocks"""
    return _second_factory("transformer_encoder_stage", model_config, dropout)


def conformer_encoder_block(model_config: dict, dropout: bool = False):
    """reference modules.conformer_encoder_block(model_config) (modules.py:410-508) -> a factory `(input_shape) -> a one-block Stage`
    (forward(x, B, training) / backward(dy, B) on [B*S, D]); configuration errors are raised here, without a device.  dropout: accept the
    library's Dropout draws (_second_factory); without it dropout_rate must be present and 0."""
    return _second_factory("conformer_encoder_block", model_config, dropout)


def conformer_encoder_stage(model_config: dict, dropout: bool = False):
    """reference modules.conformer_encoder_stage(model_config) (modules.py:129-152): `depth` blocks"""
    return _second_factory("conformer_encoder_stage", model_config, dropout)


def attention_block(model_config: dict, dropout: bool = False):
    """reference modules.attention_block(model_config) (modules.py:511-635) -> a factory `(input_shape) -> a one-block Stage`
    (forward(x, B, training) / backward(dy, B) on [B*S, D]); configuration errors are raised here, without a device.  dropout: accept the
    library's Dropout draws (_second_factory); without it dropout_rate must be present and 0."""
    return _second_factory("attention_block", model_config, dropout)


def attention_stage(model_config: dict, dropout: bool = False):
    """reference modules.attention_stage(model_config) (modules.py:155-180): `depth` blocks"""
    return _second_factory("attention_stage", model_config, dropout)


def RNN_block(model_config: dict):
    """reference modules.RNN_block(model_config) (modules.py:322-347) -> a factory `(input_shape) -> a one-block Stage` (forward(x, B, training)
    / backward(dy, B) on [B*S, D] -> [B*S, out_dim]); configuration errors are raised here, without a device."""
    return _second_factory("RNN_block", model_config)


def RNN_stage(model_config: dict):
    """reference modules.RNN_stage(model_config) (modules.py:64-83): `depth` blocks"""
    return _second_factory("RNN_stage", model_config)
