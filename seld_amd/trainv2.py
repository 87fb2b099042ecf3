"""Host-side mirror of the reference's trainv2.py step functions (trainv2.py:23-66), utils.AdaBelief / apply_kernel_regularizer
(utils.py:99-194, 343-350) and swa.SWA (swa.py).  The arithmetic — weighted losses, L2 regulariser, AGC, AdaBelief, the running
average — runs in libseld_hip.so (seld_amd/csrc/trainv2.hip); these objects select and sequence it.  Two kinds of model take the recipe: a
fused context (models.SeldNet: the seld_*_v2 entry points) and a composed model (modules.ComposedSeldNet, models.conv_temporal's
ConvTemporalNet among them: the stream operators seld_v2_losses / seld_v2_opt / seld_v2_swa on the model's flat buffers)."""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np
import torch

from . import _lib, losses, train
from .models import SeldNet
from .modules import ComposedSeldNet

# "These are statistics from the train dataset" (trainv2.py:24-29): frames per class
TRAIN_SAMPLES = (58193, 32794, 29801, 21478, 14822, 9174, 66527, 6740, 9342, 6498, 22218, 49758)
CLIP_FACTOR = 0.01      # utils.adaptive_clip_grad's default, which trainv2.trainstep takes (trainv2.py:52)


def default_cls_weights() -> np.ndarray:
    """cls_weights = reduce_mean(train_samples) / train_samples (trainv2.py:30), in float32 as the reference evaluates it."""
    t = np.asarray(TRAIN_SAMPLES, np.float32)
    return (t.mean(dtype=np.float32) / t).astype(np.float32)


class AdaBelief:
    """utils.AdaBelief(learning_rate) (utils.py:99-116; amsgrad is not built): the slots are the model's Adam slots (the HIP ctx's, or a
    composed model's flat buffers)."""

    def __init__(self, learning_rate: float = 1e-3, beta_1: float = 0.9, beta_2: float = 0.999, epsilon: float = 1e-7):
        self.learning_rate, self.beta_1, self.beta_2, self.epsilon = learning_rate, beta_1, beta_2, epsilon


def is_regularized(name: str) -> bool:
    """Which variables utils.apply_kernel_regularizer (utils.py:343-350) gives an L2 term, by the names seld_variable_info reports: the
    `kernel` of a Conv2D, Conv1D or Dense layer (conv*.kernel, rn*.kernel, sed|doa.dense*.kernel, sed|doa.out.kernel).  Not biases and
    BatchNorm variables (no kernel), not the GRU kernels (the Bidirectional wrapper has no `kernel_regularizer` attribute, so the loop
    skips it), not SeparableConv2D's depthwise_kernel / pointwise_kernel (Keras reads depthwise_ / pointwise_regularizer there)."""
    return name.endswith(".kernel") and not name.startswith("gru")


_HEAD_MAJOR = ("query_kernel", "key_kernel", "value_kernel", "projection_kernel", "pos_kernel", "pos_bias_u", "pos_bias_v")
_KERAS_MHA = ("query", "key", "value", "attention_output")


def is_regularized_composed(name: str) -> bool:
    """The same question for a composed model's variable names (modules.py; DESIGN.md §3i has the reasoning).  utils.apply_kernel_regularizer
    sets the regulariser on every layer with a public `kernel_regularizer` attribute, so regularised are
      * `*.kernel` of a Dense / Conv1D / Conv2D layer — the stem, the mother blocks' convolutions, projections and squeeze-and-excite
        pair, the conformer's feed-forward, pointwise and depthwise (a grouped Conv1D) layers, the transformer's Conv1D pair, the dense
        blocks, sed_out / doa_out — and the input `kernel` of a one-direction RNN_block (a bare GRU / LSTM layer has the attribute; its
        recurrent_kernel reads recurrent_regularizer);
      * the head-major attention layers' query_ / key_ / value_ / projection_kernel, pos_kernel, pos_bias_u and pos_bias_v
        (layers.py:123, 150-175, 336-356 pass kernel_regularizer to all of them).
    Not: biases, gamma / beta; everything under a Bidirectional wrapper (`.fwd.` / `.bwd.`: the wrapper has no such attribute); the Keras
    MultiHeadAttention of transformer_encoder_block (`mha.query|key|value|attention_output.kernel`: it keeps the regulariser in a private
    attribute under the TensorFlow the reference requires)."""
    parts = name.split(".")
    leaf = parts[-1]
    if "fwd" in parts[:-1] or "bwd" in parts[:-1]:
        return False
    if leaf in _HEAD_MAJOR:
        return True
    if leaf != "kernel":
        return False
    return not (len(parts) >= 3 and parts[-3] == "mha" and parts[-2] in _KERAS_MHA)


def _not_wired(what: str) -> ValueError:
    return ValueError(f"{what} is wired for models.seldnet / seldnet_v1 contexts and for composed models (modules.ComposedSeldNet, "
                      "models.conv_temporal), not for this object")


def apply_kernel_regularizer(model, l2: float = 0.001):
    """utils.apply_kernel_regularizer(model, l1_l2(l1=0, l2=l2)) (trainv2.py:247, 289): marks the regularised variables (in the ctx, or in
    the composed model's optimizer plan) and remembers l2 for the v2 trainstep.  Returns the model, as the reference does."""
    if not isinstance(model, (SeldNet, ComposedSeldNet)):
        raise _not_wired("the v2 recipe")
    if l2 < 0:
        raise ValueError("l2 must be >= 0")
    if isinstance(model, ComposedSeldNet):
        model.set_regularized([is_regularized_composed(n) for n, _, _ in model.variables])
        model._v2_l2 = float(l2)
        return model
    flags = (C.c_int32 * len(model.variables))(*[int(is_regularized(n)) for n, _, _ in model.variables])
    _lib.check(model.lib.seld_set_regularized(model.ctx, flags, len(model.variables)), model.ctx)
    model._v2_l2 = float(l2)
    return model


def _v2_cfg(sed_loss, loss_weights: Sequence[float], label_smoothing: float, cls_weights: np.ndarray) -> _lib.V2Cfg:
    cfg = _lib.V2Cfg()
    if isinstance(sed_loss, losses._FocalLoss):
        cfg.sed_loss, cfg.focal_alpha, cfg.focal_gamma = _lib.SELD_SED_FOCAL, sed_loss.alpha, sed_loss.gamma
    else:
        cfg.sed_loss, cfg.focal_alpha, cfg.focal_gamma = _lib.SELD_SED_BCE, 0.25, 2.0
    cfg.w_sed, cfg.w_doa, cfg.label_smoothing = float(loss_weights[0]), float(loss_weights[1]), float(label_smoothing)
    for i, w in enumerate(cls_weights):
        cfg.cls_weights[i] = float(w)
    return cfg


def generate_trainstep(sed_loss, doa_loss, loss_weights, label_smoothing: float = 0., cls_weights=None):
    """reference trainv2.generate_trainstep (trainv2.py:23-56) -> trainstep(model, x, y, optimizer) -> (y_p, sloss, dloss).
    sed_loss: losses.BinaryCrossentropy() (the reference passes K.binary_crossentropy) or losses.focal_loss; doa_loss:
    losses.MMSE_with_cls_weights.  `cls_weights`: the reference's table has twelve classes; a model with another n_classes needs its own."""
    if not isinstance(sed_loss, (losses.BinaryCrossentropy, losses._FocalLoss)):
        raise ValueError("sed_loss must be seld_amd.losses.BinaryCrossentropy() or seld_amd.losses.focal_loss")
    if not isinstance(doa_loss, losses._MMSEWithClsWeights):
        raise ValueError("doa_loss must be seld_amd.losses.MMSE_with_cls_weights")
    if not 0.0 <= float(label_smoothing) < 1.0:
        raise ValueError("label_smoothing: [0, 1)")
    given = None if cls_weights is None else np.asarray(cls_weights, np.float32).reshape(-1)
    loss_weights = (float(loss_weights[0]), float(loss_weights[1]))

    def trainstep(model, x, y, optimizer: AdaBelief):
        nc = int(getattr(model, "n_classes", -1))
        if given is None and nc != len(TRAIN_SAMPLES):
            raise ValueError(f"the reference's class-weight table has {len(TRAIN_SAMPLES)} classes, the model has {nc}: pass cls_weights=")
        w = default_cls_weights() if given is None else given
        if w.size != nc or nc > _lib.V2_MAX_CLASSES:
            raise ValueError(f"cls_weights has {w.size} entries, the model {nc} classes (at most {_lib.V2_MAX_CLASSES})")
        if isinstance(model, ComposedSeldNet):
            return model.train_step_v2(x, y, _v2_cfg(sed_loss, loss_weights, label_smoothing, w), optimizer, float(getattr(model, "_v2_l2", 0.0)),
                                       CLIP_FACTOR)
        if not isinstance(model, SeldNet):
            raise _not_wired("the v2 trainstep")
        x = model._prep(x)
        B = x.shape[0]
        ys, yd = train._labels(model, y, B)
        sed, doa = model._outputs(B)
        sloss = torch.empty((), dtype=torch.float32, device=model._dev)
        dloss = torch.empty((), dtype=torch.float32, device=model._dev)
        cfg = _v2_cfg(sed_loss, loss_weights, label_smoothing, w)
        _lib.check(model.lib.seld_train_fwd_bwd_v2(model.ctx, x.data_ptr(), ys.data_ptr(), yd.data_ptr(), C.byref(cfg), sed.data_ptr(),
                                                   doa.data_ptr(), sloss.data_ptr(), dloss.data_ptr()), model.ctx)
        _lib.check(model.lib.seld_v2_opt_step(model.ctx, optimizer.learning_rate, optimizer.beta_1, optimizer.beta_2, optimizer.epsilon,
                                              float(getattr(model, "_v2_l2", 0.0)), CLIP_FACTOR), model.ctx)
        return [sed, doa], sloss, dloss
    return trainstep


def generate_teststep(sed_loss, doa_loss):
    """reference trainv2.generate_teststep (trainv2.py:59-66) -> teststep(model, x, y, optimizer=None).  There sed_loss returns the
    elementwise tensor that the loop's Mean metric averages, and doa_loss is called without weights: mean BCE and plain MMSE, which is
    train.teststep with losses.MMSE.  A focal sed_loss has no unweighted test kernel."""
    if not isinstance(sed_loss, losses.BinaryCrossentropy):
        raise ValueError("the v2 test step is built for sed_loss = seld_amd.losses.BinaryCrossentropy()")
    if not isinstance(doa_loss, (losses._MMSEWithClsWeights, losses._MMSE)):
        raise ValueError("doa_loss must be seld_amd.losses.MMSE_with_cls_weights")

    def teststep(model, x, y, optimizer=None):
        if not isinstance(model, (SeldNet, ComposedSeldNet)):
            raise _not_wired("the v2 test step")
        return train.teststep(model, x, y, sed_loss, losses.MMSE)
    return teststep


class SWA:
    """swa.SWA (swa.py): the running average lives in the HIP ctx, or in a composed model's own buffers (weights and BatchNorm moving
    statistics, as model.get_weights() holds both)."""

    def __init__(self, model, start_epoch: int, swa_freq: int = 2, verbose: bool = False):
        if not isinstance(model, (SeldNet, ComposedSeldNet)):
            raise _not_wired("SWA")
        self.model, self.start_epoch, self.swa_freq, self.verbose = model, start_epoch - 1, swa_freq, verbose
        self._composed = isinstance(model, ComposedSeldNet)

    @property
    def cnt(self) -> int:
        if self._composed:
            return self.model.swa_count
        return int(self.model.lib.seld_swa_count(self.model.ctx))

    def on_epoch_end(self, epoch: int) -> None:
        epoch = epoch - self.start_epoch
        if epoch == 0 or (epoch > 0 and epoch % self.swa_freq == 0):      # swa.py:14-19
            if self.verbose:
                print("\nSaving Weights... ", epoch + self.start_epoch)
            self.update_swa_weights()

    def update_swa_weights(self) -> None:
        if self._composed:
            return self.model.swa_update()
        _lib.check(self.model.lib.seld_swa_update(self.model.ctx), self.model.ctx)

    def on_train_end(self) -> None:
        if self._composed:
            return self.model.swa_apply()
        _lib.check(self.model.lib.seld_swa_apply(self.model.ctx), self.model.ctx)
