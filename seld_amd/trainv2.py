"""Host-side mirror of the reference's trainv2.py step functions (trainv2.py:23-66), utils.AdaBelief / apply_kernel_regularizer
(utils.py:99-194, 343-350) and swa.SWA (swa.py).  The arithmetic — weighted losses, L2 regulariser, AGC, AdaBelief, the running
average — runs in libseld_hip.so (seld_amd/csrc/trainv2.hip); these objects select and sequence it.  Two kinds of model take the recipe: a
fused context (models.SeldNet: the seld_*_v2 entry points) and a composed model (modules.ComposedSeldNet, models.conv_temporal's
ConvTemporalNet among them: the stream operators seld_v2_losses / seld_v2_opt / seld_v2_swa on the model's flat buffers).

Around the step: get_dataset (trainv2.py:127-155), generate_iterloop (:69-117), generate_evaluate_fn (:195-237; the DCASE score of the
sliding-window outputs on the device, SELD_evaluation_metrics.SELDMetrics_) and main (:240-369):
    python -m seld_amd.trainv2 --name x --model conv_temporal --model_config SS5 --abspath DATA/ --ans_path METADATA_DEV/"""
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


# ---------------------------------------------------------------------------------------------------
WIN_SIZE, STEP_SIZE = 300, 5      # ensemble_outputs' defaults (trainv2.py:158-159): 300-frame windows every 5 frames, one label frame per 5


def get_dataset(config, mode: str = 'train', device=None):
    """reference trainv2.get_dataset (trainv2.py:127-155).  --use_tfm: random_ups_and_downs, ten time masks and six frequency masks in one
    kernel (transforms.v2_sample_transforms); --use_acs: foa_intensity_vec_aug — both on the device batch of the train set, in the
    reference's order, applied by the step loop as train.get_dataset wires its transforms.  `device`: keep the windowed dataset in that
    GPU's HBM."""
    import os
    from . import data_loader as dl, transforms as tfm
    path = os.path.join(config.abspath, 'DCASE2021/feat_label/')
    x, y = dl.load_seldnet_data(os.path.join(path, 'foa_dev_norm'), os.path.join(path, 'foa_dev_label'), mode=mode, n_freq_bins=64)
    device_transforms = []
    if getattr(config, 'use_tfm', False) and mode == 'train':
        device_transforms.append(lambda x, y, rng: (tfm.v2_sample_transforms(x, rng=rng), y))
    if getattr(config, 'use_acs', False) and mode == 'train':
        device_transforms.append(lambda x, y, rng: tfm.foa_intensity_vec_aug(x, y, rng=rng))
    ds = dl.seldnet_data_to_dataloader(x, y, train=mode == 'train', label_window_size=60, batch_size=config.batch,
                                       loop_time=config.loop_time, device_transforms=device_transforms)
    return ds.to_device(device) if device is not None else ds


def generate_iterloop(sed_loss, doa_loss, evaluator, mode, loss_weights=None, label_smoothing=0.):
    """reference trainv2.generate_iterloop (trainv2.py:69-117) -> iterloop(model, dataset, epoch, optimizer=None) -> (mean sed loss, mean
    doa loss, seld score).  `evaluator` (seld_amd.metrics.SELDMetrics) is reset, then updated on the device after every step; the losses
    are summed on the device: one host synchronisation per epoch.  The progress bar and the tensorboard writer are left out."""
    from . import metrics as _metrics
    if mode == 'train':
        if loss_weights is None:
            raise ValueError("the train loop needs loss_weights")
        step = generate_trainstep(sed_loss, doa_loss, loss_weights, label_smoothing)
    else:
        step = generate_teststep(sed_loss, doa_loss)

    def iterloop(model, dataset, epoch, optimizer=None):
        evaluator.reset_states()
        tot_s = torch.zeros((), device=model._dev)
        tot_d = torch.zeros((), device=model._dev)
        n = 0
        dev_tf = getattr(dataset, 'device_transforms', None)
        for x, y in dataset:
            if dev_tf:        # augmentation on the device batch; labels arrive unsplit [b,60,4C] (data_loader.SeldDataset)
                x = torch.as_tensor(x, dtype=torch.float32).to(model._dev).contiguous()
                y = torch.as_tensor(y, dtype=torch.float32).to(model._dev).contiguous()
                for f in dev_tf:
                    x, y = f(x, y, dataset.rng)
                nc = y.shape[-1] // 4
                y = (y[..., :nc].contiguous(), y[..., nc:].contiguous())
            preds, sloss, dloss = step(model, x, y, optimizer)
            evaluator.update_states(y, preds)
            tot_s += sloss
            tot_d += dloss.mean()
            n += 1
        score = _metrics.calculate_seld_score(evaluator.result())
        return float(tot_s.item()) / max(n, 1), float(tot_d.item()) / max(n, 1), score
    return iterloop


def _label_frames(n_frames: int, win_size: int = WIN_SIZE, step_size: int = STEP_SIZE) -> int:
    """label frames ensemble_outputs returns for a clip of n_frames feature frames: (windows - 1) + win_size // step_size"""
    return (n_frames - win_size) // step_size + win_size // step_size


def generate_evaluate_fn(test_xs, test_labels, write_path, ans_path=None, batch_size=256, doa_threshold=20, nb_classes=12):
    """reference trainv2.generate_evaluate_fn (trainv2.py:195-237) -> evaluate_fn(model, epoch) -> (seld_score, (ER, F, LE, LR)).

    evaluate_fn: ensemble_outputs on every test clip, then — when `write_path` is not None — utils.write_answer of `sed > 0.5` per file,
    then ONE SELDMetrics_.update_seld_scores over all files (the reference scores file by file from the csv it has just written), then
    compute_seld_scores and metrics.calculate_seld_score.  The reference's SELDMetrics_() keeps its default of 11 classes and so never looks
    at the twelfth; `nb_classes` is explicit here.

    Ground truth, with `ans_path`: as trainv2.py:202-213 reads it — sorted `ans_path/dev-test/*`, the files whose name carries fold digit 6
    at index 4, polar -> cartesian, paired by position with `test_xs` (the two lists must be equally long, which the reference does not
    check).  Without it, `test_labels` holds the already loaded cartesian dicts.  Either way the labels are packed once, here."""
    import os
    from glob import glob
    from . import utils
    if ans_path is not None:
        files = sorted(glob(os.path.join(ans_path, 'dev-test', '*')))
        files = [f for f in files if int(os.path.basename(f)[4]) in [6]]
        names = [os.path.splitext(os.path.basename(f))[0] for f in files]
        dicts = [utils.convert_output_format_polar_to_cartesian(utils.load_output_format_file(f)) for f in files]
    else:
        if test_labels is None:
            raise ValueError("generate_evaluate_fn needs ans_path or the loaded label dicts")
        dicts = list(test_labels)
        names = [f'fold6_file{i:03d}' for i in range(len(dicts))]
    if len(dicts) != len(test_xs):
        raise AssertionError(f"{len(test_xs)} test clips but {len(dicts)} label files: they are paired by position")
    packed = utils.concat_labels([utils.pack_labels(d, _label_frames(int(np.shape(x)[0])), nb_classes) for d, x in zip(dicts, test_xs)])

    def evaluate_fn(model, epoch):
        from . import evaluator as _evaluator, metrics as _metrics
        from .SELD_evaluation_metrics import SELDMetrics_
        e_outs = _evaluator.ensemble_outputs(model, test_xs, win_size=WIN_SIZE, step_size=STEP_SIZE, batch_size=batch_size)
        if write_path is not None:
            os.makedirs(write_path, exist_ok=True)
            for name, (sed, doa) in zip(names, e_outs):
                utils.write_answer(write_path, name + '.csv', sed > 0.5, doa)
        seld_ = SELDMetrics_(doa_threshold=doa_threshold, nb_classes=nb_classes, device=model._dev)
        seld_.update_seld_scores(e_outs, packed, sed_thresh=0.5)
        metric_values = seld_.compute_seld_scores()
        seld_score = float(_metrics.calculate_seld_score(metric_values))
        er, f, der, derf = metric_values
        print(f'ensemble outputs (epoch {epoch})  ER: {er:4f}, F: {f:4f}, DER: {der:4f}, DERF: {derf:4f}, SELD: {seld_score:4f}')
        return seld_score, metric_values
    evaluate_fn.names = names
    return evaluate_fn


def main(config, model_config=None, max_epochs=None, swa_start_epoch=80, swa_freq=2, eval_every=10, l2=0.001, label_smoothing=0.):
    """reference trainv2.main (trainv2.py:240-369): datasets, a model with n_classes = 12 built for the largest batch any pass uses, L2
    flags, AdaBelief, BCE + MMSE_with_cls_weights, SWA, `--resume` from the saved .npz weights, then per epoch: halve the learning rate at
    `swa_start_epoch`, evaluate_fn every `eval_every` epochs, the train / val / test loops, swa.on_epoch_end, best model by validation
    score, early stop on config.patience (the reference's LR-on-plateau block is commented out and is left out); at the end
    swa.on_train_end(), a last evaluate_fn and `SWA_best_{score:.5f}.npz`.  -> (model, history)."""
    import os
    from . import data_loader as dl, metrics as _metrics, models
    if isinstance(config, tuple):
        config, model_config = config
    if config.sed_loss != 'BCE':
        raise ValueError("trainv2.main: sed_loss must be 'BCE' (generate_teststep has no focal test kernel)")
    if model_config is None:
        raise ValueError("trainv2.main needs the model configuration")
    if not callable(getattr(models, config.model, None)) or config.model.startswith('_'):
        raise ValueError(f"seld_amd.models has no model {config.model!r}")
    if swa_freq < 1 or eval_every < 1 or swa_start_epoch < 1:
        raise ValueError("swa_start_epoch, swa_freq and eval_every must be at least 1")
    loss_weights = [int(i) for i in config.loss_weight.split(',')]
    if len(loss_weights) != 2:
        raise ValueError("--loss_weight takes two comma-separated integers")
    n_classes = 12                                                  # trainv2.py:244
    dev = torch.device('cuda', torch.cuda.current_device())
    trainset, valset, testset = (get_dataset(config, m, dev) for m in ('train', 'val', 'test'))      # HBM-resident
    path = os.path.join(config.abspath, 'DCASE2021/feat_label/')
    test_xs, _ = dl.load_seldnet_data(os.path.join(path, 'foa_dev_norm'), os.path.join(path, 'foa_dev_label'), mode='test', n_freq_bins=64)
    x, y = next(iter(trainset.take(1)))
    input_shape = (max(config.batch, valset.batch_size, testset.batch_size),) + tuple(x.shape[1:])
    model_config = dict(model_config)
    model_config['n_classes'] = n_classes
    model = getattr(models, config.model)(input_shape, model_config)
    model.summary()
    model = apply_kernel_regularizer(model, l2)
    optimizer = AdaBelief(config.lr)
    sed_loss = losses.BinaryCrossentropy()
    doa_loss = losses.MMSE_with_cls_weights                         # trainv2.py:296-297
    swa = SWA(model, swa_start_epoch, swa_freq)
    model_path = os.path.join('./saved_model', config.name)
    os.makedirs(model_path, exist_ok=True)
    if getattr(config, 'resume', False):                           # trainv2.py:302-306: the saved model's weights
        from glob import glob
        saved = sorted(glob(os.path.join(model_path, '*.npz')))
        if len(saved) == 0:
            raise ValueError('the model does not exist, cannot be resumed')
        model.load_weights(saved[0])
    evaluator = _metrics.SELDMetrics(doa_threshold=config.lad_doa_thresh, n_classes=n_classes)
    train_iterloop = generate_iterloop(sed_loss, doa_loss, evaluator, 'train', loss_weights=loss_weights, label_smoothing=label_smoothing)
    val_iterloop = generate_iterloop(sed_loss, doa_loss, evaluator, 'val')
    test_iterloop = generate_iterloop(sed_loss, doa_loss, evaluator, 'test')
    evaluate_fn = generate_evaluate_fn(test_xs, None, config.output_path, config.ans_path, config.batch * 4,
                                       doa_threshold=config.lad_doa_thresh, nb_classes=n_classes)
    best, early, history, epoch = float('inf'), 0, [], 0
    for epoch in range(config.epoch if max_epochs is None else min(config.epoch, max_epochs)):
        if epoch == swa_start_epoch:
            optimizer.learning_rate = config.lr * 0.5              # trainv2.py:325-326
        ev = evaluate_fn(model, epoch) if epoch % eval_every == 0 else None
        tr = train_iterloop(model, trainset, epoch, optimizer)
        va = val_iterloop(model, valset, epoch)
        te = test_iterloop(model, testset, epoch)
        score = va[2]
        swa.on_epoch_end(epoch)
        history.append({'epoch': epoch, 'train': tr, 'val': va, 'test': te, 'score': score, 'lr': optimizer.learning_rate, 'eval': ev})
        print(f'epoch {epoch}: train sed/doa/seld {tr[0]:.4f}/{tr[1]:.5f}/{tr[2]:.4f}  val {va[0]:.4f}/{va[1]:.5f}/{va[2]:.4f}'
              f'  test {te[0]:.4f}/{te[1]:.5f}/{te[2]:.4f}')
        if best > score:                                            # trainv2.py:338-346
            old = os.path.join(model_path, f'bestscore_{best}.npz')
            if os.path.exists(old):
                os.remove(old)
            best, early = score, 0
            model.save_weights(os.path.join(model_path, f'bestscore_{best}.npz'))
        else:                                                       # trainv2.py:347-358
            if early == config.patience:
                print(f'Early Stopping at {epoch}, score is {score}')
                break
            early += 1
    print(f'epoch: {epoch}')
    if swa.cnt > 0:
        swa.on_train_end()
    seld_score, _ = evaluate_fn(model, epoch)
    model.save_weights(os.path.join(model_path, f'SWA_best_{seld_score:.5f}.npz'))
    return model, history


if __name__ == '__main__':
    from . import params
    main(params.get_param())
