"""Host-side mirror of the reference's train.py step functions (train.py:22-44) plus the
data-parallel wrapper the reference lacks, its datasets and its epoch loop.

--use_tdm (train.py:210-261, 279-288, 341-356): get_tdm_dataset regenerates the training set on the device from a TdmSource (clean waves,
labels and the noise bank, resident in HBM).  Deviations from the reference: the draws come from a numpy Generator `rng` (or an explicit
plan `draws`), not TensorFlow's; the bank is read from .npy, not .joblib; the three hard-coded paths are flags (--tdm_wav_path,
--tdm_label_path, --tdm_bank_path); the features come from the library's extractor, the one that produced foa_dev_norm, not from the
reference's separate TF re-implementation get_preprocessed_x_tf (which differs from it and from the validation features); n_classes is a
parameter, and main refuses labels whose class count is not the model's.

    python -m seld_amd.train --name x --abspath DATA/ --use_tdm --tdm_wav_path FOA_DEV/ --tdm_label_path METADATA_DEV/ --tdm_bank_path BANK/"""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import torch

from . import _lib, losses, parallel
from .models import SeldNet


class Adam:
    """tf.keras.optimizers.Adam(learning_rate) (train.py:311): the slots live in the HIP ctx."""

    def __init__(self, learning_rate: float = 1e-3, beta_1: float = 0.9, beta_2: float = 0.999, epsilon: float = 1e-7):
        self.learning_rate, self.beta_1, self.beta_2, self.epsilon = learning_rate, beta_1, beta_2, epsilon


def _cfg(doa_loss, loss_weight: Sequence[float], sed_grad_scale: float = 1.0, mmse_den: float = 0.0) -> _lib.LossCfg:
    if not isinstance(doa_loss, (losses._MSE, losses._MMSE)):
        raise ValueError("doa_loss must be seld_amd.losses.MSE, .MAE, .MSLE or .MMSE")
    return _lib.LossCfg(doa_loss.code, float(loss_weight[0]), float(loss_weight[1]), float(sed_grad_scale), float(mmse_den))


def _labels(model: SeldNet, y, B: int):
    ys = torch.as_tensor(y[0], dtype=torch.float32, device=model._dev).contiguous()
    yd = torch.as_tensor(y[1], dtype=torch.float32, device=model._dev).contiguous()
    if tuple(ys.shape) != (B, model.S, model.n_classes) or tuple(yd.shape) != (B, model.S, 3 * model.n_classes):
        raise ValueError(f"label shapes {tuple(ys.shape)}, {tuple(yd.shape)} do not match the model output")
    return ys, yd


def _loss_outputs(model: SeldNet, doa_loss, B: int):
    sloss = torch.empty((), dtype=torch.float32, device=model._dev)
    dshape = (B, model.S) if isinstance(doa_loss, losses._MSE) else ()
    dloss = torch.empty(dshape, dtype=torch.float32, device=model._dev)
    return sloss, dloss


def trainstep(model: SeldNet, x, y, sed_loss, doa_loss, loss_weight, optimizer: Adam, agc: bool = False,
              process_group=None, allreduce: bool = True):
    """reference train.trainstep (train.py:22-36) -> (y_p, sloss, dloss).

    With torch.distributed initialised (one process per GPU) the flat gradient buffer is summed over
    ranks with one RCCL all-reduce between backward and Adam; BatchNorm statistics stay per replica."""
    if not isinstance(sed_loss, losses.BinaryCrossentropy):
        raise ValueError("sed_loss must be seld_amd.losses.BinaryCrossentropy()")
    if not isinstance(model, SeldNet):       # modules.ComposedSeldNet (FIRST = mother_block / mother_stage): single process
        if parallel.world_size(process_group) > 1:
            raise ValueError("composed models are not data-parallel")
        return model.train_step(x, y, _cfg(doa_loss, loss_weight), optimizer, agc)
    x = model._prep(x)
    B = x.shape[0]
    ys, yd = _labels(model, y, B)
    sed, doa = model._outputs(B)
    sloss, dloss = _loss_outputs(model, doa_loss, B)
    world = parallel.world_size(process_group)
    is_mmse = isinstance(doa_loss, losses._MMSE)
    lib_dp = getattr(model, "_lib_dp", False)        # parallel.init_library_dp: the library owns the RCCL communicator
    if world > 1 and not lib_dp and not getattr(model, "_dp_seeded", False):
        # torch.distributed path: every replica needs its own dropout key too (init_library_dp sets it on the library path), or all
        # ranks would drop the same elements of their different clips
        model.set_option("dropout_seed", 0x5e1d + torch.distributed.get_rank(process_group))
        model._dp_seeded = True
    dent = None
    if lib_dp:
        pass            # the mask count is all-reduced on the device inside seld_train_fwd_bwd (cfg.mmse_den = 0)
    elif world > 1 and is_mmse:
        # scalar objective: BCE is a mean over the GLOBAL batch, MMSE divides by the GLOBAL sum(mask)
        dent = torch.empty(1, dtype=torch.float32, device=model._dev)
        _lib.check(model.lib.seld_mmse_den(model.ctx, yd.data_ptr(), dent.data_ptr()), model.ctx)
    if lib_dp:
        sed_scale, den = (1.0 / int(model.lib.seld_dp_world(model.ctx)) if is_mmse else 1.0), 0.0
    else:
        sed_scale, den = parallel.loss_scaling(is_mmse, dent, process_group)
    cfg = _cfg(doa_loss, loss_weight, sed_scale, den)
    _lib.check(model.lib.seld_train_fwd_bwd(model.ctx, x.data_ptr(), ys.data_ptr(), yd.data_ptr(), C.byref(cfg),
                                            sed.data_ptr(), doa.data_ptr(), sloss.data_ptr(), dloss.data_ptr()), model.ctx)
    if (world > 1 or lib_dp) and allreduce:      # allreduce=False: timing aid only (bench.py measures the exposed communication time with it)
        parallel.allreduce_gradients(model.grad_tensor(), process_group, model)
    _lib.check(model.lib.seld_adam_step(model.ctx, optimizer.learning_rate, optimizer.beta_1, optimizer.beta_2,
                                        optimizer.epsilon, int(bool(agc))), model.ctx)
    return [sed, doa], sloss, dloss


def teststep(model: SeldNet, x, y, sed_loss, doa_loss):
    """reference train.teststep (train.py:39-44) -> (y_p, sloss, dloss)."""
    if not isinstance(model, SeldNet):       # modules.ComposedSeldNet
        return model.test_step(x, y, _cfg(doa_loss, (1.0, 1.0)))
    x = model._prep(x)
    B = x.shape[0]
    ys, yd = _labels(model, y, B)
    sed, doa = model._outputs(B)
    sloss, dloss = _loss_outputs(model, doa_loss, B)
    cfg = _cfg(doa_loss, (1.0, 1.0))
    _lib.check(model.lib.seld_test_step(model.ctx, x.data_ptr(), ys.data_ptr(), yd.data_ptr(), C.byref(cfg),
                                        sed.data_ptr(), doa.data_ptr(), sloss.data_ptr(), dloss.data_ptr()), model.ctx)
    return [sed, doa], sloss, dloss


# ---------------------------------------------------------------------------------------------------
def get_dataset(config, mode: str = 'train', device=None):
    """reference train.get_dataset (train.py:150-176).  `device`: keep the windowed dataset resident in that GPU's HBM
    (batches are device-side gathers; what `main` does) instead of yielding numpy batches.  --use_tfm: time and frequency masks (transforms.mask, per
    sample and per 100-frame segment); --use_acs: foa_intensity_vec_aug on the batch — both on the device
    (seld_amd.transforms), applied by `iterloop` to the batch after its host->HBM copy."""
    import os
    from . import data_loader as dl
    path = os.path.join(config.abspath, 'DCASE2021/feat_label/')
    x, y = dl.load_seldnet_data(os.path.join(path, 'foa_dev_norm'), os.path.join(path, 'foa_dev_label'), mode=mode, n_freq_bins=64)
    device_transforms = _train_transforms(config) if mode == 'train' else []
    ds = dl.seldnet_data_to_dataloader(x, y, train=mode == 'train', label_window_size=60, batch_size=config.batch,
                                       loop_time=config.loop_time, device_transforms=device_transforms)
    return ds.to_device(device) if device is not None else ds


def _train_transforms(config):
    """the device transforms --use_tfm and --use_acs attach to a training set (train.py:157-165, 240-251)"""
    from . import transforms as tfm
    device_transforms = []
    if getattr(config, 'use_tfm', False):
        device_transforms.append(lambda x, y, rng: (tfm.mask(x, -3, max_mask_size=config.time_mask_size, rng=rng), y))
        device_transforms.append(lambda x, y, rng: (tfm.mask(x, -2, max_mask_size=config.freq_mask_size, rng=rng), y))
    if getattr(config, 'use_acs', False):
        device_transforms.append(lambda x, y, rng: tfm.foa_intensity_vec_aug(x, y, rng=rng))
    return device_transforms


class TdmSource:
    """What every regeneration of the time-domain-mixed training set starts from, resident in HBM: the clean waves [n, C, N] (the DCASE train
    split: 400 clips x 5.76 MB x 4 channels = 9.2 GB), their labels [n, T, 4*nc] and the packed noise bank (data_loader.TdmBank).  Loaded once;
    get_tdm_dataset mixes out of place, so the waves stay clean.  `regenerations` counts the datasets made from it."""

    def __init__(self, x, y, tdm_x, tdm_y=None, sr=24000, label_resolution=0.1, device=None):
        import numpy as np
        from . import data_loader as dl
        dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        if isinstance(x, (list, tuple)):
            if len({tuple(w.shape) for w in x}) != 1:
                raise ValueError('time-domain mixing needs clips of one length (the reference stacks them too, train.py:237)')
            x = np.stack([np.asarray(w, np.float32) for w in x]) if not isinstance(x[0], torch.Tensor) else torch.stack(list(x))
        if isinstance(y, (list, tuple)):
            y = np.stack([np.asarray(l, np.float32) for l in y]) if not isinstance(y[0], torch.Tensor) else torch.stack(list(y))
        self.x = torch.as_tensor(x, dtype=torch.float32).to(dev).contiguous()
        self.y = torch.as_tensor(y, dtype=torch.float32).to(dev).contiguous()
        self.bank = tdm_x if isinstance(tdm_x, dl.TdmBank) else dl.TdmBank(tdm_x, tdm_y, sr, label_resolution, dev)
        self.sr, self.label_resolution = sr, label_resolution
        if self.x.dim() != 3 or self.y.dim() != 3 or self.x.shape[0] != self.y.shape[0] or self.x.shape[2] < self.y.shape[1] * self.bank.spf:
            raise ValueError(f'waves {tuple(self.x.shape)} and labels {tuple(self.y.shape)} must be [n, C, N >= T * {self.bank.spf}] and [n, T, 4 * n_classes]')
        if self.y.shape[2] != self.bank.W or self.x.shape[1] != self.bank.C:
            raise ValueError(f'the bank ({self.bank.C} channels, labels {self.bank.W} wide) does not match the clips '
                             f'({self.x.shape[1]} channels, labels {self.y.shape[2]} wide)')
        self.device = dev
        self.extractor = None
        self.regenerations = 0

    @classmethod
    def load(cls, config, n_classes=12, max_label_length=600, device=None):
        """train.get_tdm_dataset's loading part (train.py:211-223), from --tdm_wav_path, --tdm_label_path and --tdm_bank_path"""
        from . import data_loader as dl
        x, y = dl.load_wav_and_label(config.tdm_wav_path, config.tdm_label_path, 'train', n_classes=n_classes, max_label_length=max_label_length)
        if not x:
            raise ValueError(f'no train-split wav files under {config.tdm_wav_path}')
        tdm_x, tdm_y = dl.get_TDMset(config.tdm_bank_path)
        return cls(x, y, tdm_x, tdm_y, device=device)


def get_tdm_dataset(config, max_overlap_num=5, max_overlap_per_frame=2, min_overlap_sec=1, max_overlap_sec=5, source=None, rng=None,
                    norm=None, chunk=32):
    """reference train.get_tdm_dataset (train.py:210-261) -> a device-resident SeldDataset of the mixed training split.

    Per chunk of `chunk` clips: seld_aug_tdm_labels on a copy of the labels, seld_aug_tdm_mix out of place into a chunk buffer, then the
    library's FeatureExtractor.batch with the reference's call parameters (n_fft = win_length = 1024, hop_length = 480, 64 mels, foa), padded or
    trimmed to 5 frames per label.  Normalisation as train.py:238: mean and population std over the CLIP axis per (frame, freq, chan), no
    eps, the sums in float64; or, with norm = (mean, std) per (freq, chan), apply_normalizer's (seld_feat_normalize, eps 1e-8) for a
    validation set that calculate_statistics normalised.  Then windows of 60 labels / 300 frames, and the device transforms of get_dataset.
    `source` (TdmSource) is loaded from the config's paths when absent; `rng` makes the draws (data_loader.draw_tdm)."""
    import numpy as np
    from . import data_loader as dl
    from .feature_extractor import FeatureExtractor
    if source is None:
        source = TdmSource.load(config)
    rng = rng or np.random.default_rng()
    lib = _lib.load()
    n, Cc, N = source.x.shape
    T = int(source.y.shape[1])
    plan = dl.draw_tdm(rng, n, T, source.bank.rows, int(max_overlap_num), dl.tdm_frames(min_overlap_sec, source.label_resolution),
                       dl.tdm_frames(max_overlap_sec, source.label_resolution))
    if source.extractor is None:
        source.extractor = FeatureExtractor(source.sr, 'foa', 64, n_fft=1024, win_length=1024, hop_length=480, device=source.device.index)
    fe = source.extractor
    frames = T * 5
    y = source.y.clone()
    st = lambda: C.c_void_p(torch.cuda.current_stream(source.device).cuda_stream)
    feats = torch.zeros((n, frames, fe.n_mels, fe.channels), dtype=torch.float32, device=source.device)
    FC = fe.n_mels * fe.channels
    if norm is not None:
        as_dev = lambda a: torch.as_tensor(np.asarray(a, np.float32) if not isinstance(a, torch.Tensor) else a).to(source.device, torch.float32).reshape(-1).contiguous()
        mean, std = as_dev(norm[0]), as_dev(norm[1])
        if mean.numel() != FC or std.numel() != FC:
            raise ValueError(f'norm = (mean, std) must have freq * chan = {FC} elements each')
    else:
        acc = torch.zeros((2, frames * FC), dtype=torch.float64, device=source.device)
    chunk = max(1, min(int(chunk), n))
    mixed = torch.empty((chunk, Cc, N), dtype=torch.float32, device=source.device)
    for i in range(0, n, chunk):
        c = min(chunk, n - i)
        dl.tdm_apply(source.x[i:i + c], mixed[:c], y[i:i + c], source.bank, plan[i:i + c], max_overlap_per_frame)
        f = fe.batch(mixed[:c])                                   # [c, 1 + N // hop, mels, chan]
        keep = min(frames, f.shape[1])                             # preprocess_features_labels: trim, or zero-pad (feats starts as zeros)
        if norm is not None:
            fk = f[:, :keep].contiguous()
            out = torch.empty_like(fk)
            _lib.check(lib.seld_feat_normalize(fk.data_ptr(), mean.data_ptr(), std.data_ptr(), out.data_ptr(), c * keep, c * keep, FC, 1e-8, st()))
            feats[i:i + c, :keep] = out
            if keep < frames:      # apply_normalizer runs behind the padding: a padded frame is (0 - mean) / std
                feats[i:i + c, keep:] = (-mean / torch.clamp(std, min=1e-8)).reshape(fe.n_mels, fe.channels)
        else:
            feats[i:i + c, :keep] = f[:, :keep]
            d = feats[i:i + c].reshape(c, -1).double()
            acc[0] += d.sum(0)
            acc[1] += (d * d).sum(0)
    if norm is None:
        m64 = acc[0] / n
        mean = m64.float()
        std = torch.sqrt(torch.clamp(acc[1] / n - m64 * m64, min=0.0)).float()
        tmp = torch.empty((chunk, frames * FC), dtype=torch.float32, device=source.device)
        for i in range(0, n, chunk):      # (x - mean) / std with the clips as rows: std = 0 gives the reference's inf / nan
            c = min(chunk, n - i)
            tmp[:c] = feats[i:i + c].reshape(c, -1)
            _lib.check(lib.seld_feat_normalize(tmp.data_ptr(), mean.data_ptr(), std.data_ptr(), feats[i:i + c].data_ptr(), c, c, frames * FC, 0.0, st()))
    n_samples = (n * T) // 60                                      # seldnet_data_to_dataloader: the clips end to end, windows of 60 labels
    x_w = feats.reshape(-1, fe.n_mels, fe.channels)[:n_samples * 300].reshape(n_samples, 300, fe.n_mels, fe.channels)
    y_w = y.reshape(-1, y.shape[2])[:n_samples * 60].reshape(n_samples, 60, y.shape[2])
    source.regenerations += 1
    ds = dl.SeldDataset(x_w, y_w, config.batch, True, config.loop_time, n_samples // config.batch, None, _train_transforms(config))
    ds.tdm_plan, ds.tdm_labels, ds.tdm_norm = plan, y, (mean, std)
    return ds


def iterloop(model: SeldNet, dataset, sed_loss, doa_loss, metric_class, config, optimizer=None, mode='train',
             process_group=None):
    """The step loop of reference train.iterloop (train.py:47-147) -> (mean sed loss, mean doa loss, seld score).
    `metric_class` (seld_amd.metrics.SELDMetrics or None) is updated on the device after every step, as the
    reference does on the host (train.py:82-83); csv dumps / DCASE official metrics / tensorboard
    (train.py:85-145) are outside the accelerated path.  One host sync per epoch instead of one per step."""
    from . import metrics as _metrics
    loss_weight = [int(i) for i in config.loss_weight.split(',')]
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
        if mode == 'train':
            preds, sloss, dloss = trainstep(model, x, y, sed_loss, doa_loss, loss_weight, optimizer, config.agc, process_group)
        else:
            preds, sloss, dloss = teststep(model, x, y, sed_loss, doa_loss)
        if metric_class is not None:
            metric_class.update_states(y, preds)
        tot_s += sloss
        tot_d += dloss.mean()
        n += 1
    score = _metrics.calculate_seld_score(metric_class.result()) if metric_class is not None else float('nan')
    return float(tot_s.item()) / max(n, 1), float(tot_d.item()) / max(n, 1), score


def main(config, model_config=None, max_epochs=None, tdm_source=None):
    """reference train.main (train.py:264-390) around the accelerated steps: datasets (train / val / test folds), model with
    n_classes forced to 12, `--resume` from the saved weights, Adam, BCE + MSE|MMSE, SELDMetrics, and the epoch loop —
    train, validation and evaluation passes — with best-model save, LR decay on plateau and early stopping on the
    validation SELD score (block-wise metrics.SELDMetrics score; the reference's csv-based DCASE scorer is out of scope).
    --use_tdm: the training set is regenerated by get_tdm_dataset on the reference's schedule (train.py:279-288, 341-356) from `tdm_source`
    (a TdmSource; loaded once from --tdm_wav_path / --tdm_label_path / --tdm_bank_path when absent).  The reference also builds a set before
    the loop that its epoch 0 replaces unseen; here that one set serves epoch 0."""
    import os
    from . import metrics as _metrics
    from . import models
    if isinstance(config, tuple):
        config, model_config = config
    dev = torch.device('cuda', torch.cuda.current_device())
    n_classes = 12                                                  # train.py:306-307
    use_tdm = getattr(config, 'use_tdm', False)
    if use_tdm:
        if tdm_source is None:
            tdm_source = TdmSource.load(config, n_classes=n_classes, device=dev)
        if tdm_source.y.shape[2] // 4 != n_classes:
            raise ValueError(f'--use_tdm: the labels hold {tdm_source.y.shape[2] // 4} classes, the model is built for {n_classes}')
        overlap_num, overlap_sec, max_overlap_num, max_overlap_sec = 1, 1, 3, 3          # train.py:280-283
        tdm_set = lambda: get_tdm_dataset(config, max_overlap_num=overlap_num, max_overlap_per_frame=2, min_overlap_sec=0.5,
                                          max_overlap_sec=overlap_sec, source=tdm_source)
        trainset, tdm_fresh = tdm_set(), True
    else:
        trainset = get_dataset(config, 'train', dev)                                          # HBM-resident
    valset = get_dataset(config, 'val', dev)
    testset = get_dataset(config, 'test', dev)                                                # train.py:290 (fold 6)
    x, y = next(iter(trainset.take(1)))
    input_shape = (max(config.batch, valset.batch_size, testset.batch_size),) + tuple(x.shape[1:])
    model_config = dict(model_config)
    model_config['n_classes'] = n_classes
    model = getattr(models, config.model)(input_shape, model_config)
    model.summary()
    optimizer = Adam(config.lr)
    sed_loss = losses.BinaryCrossentropy()
    doa_loss = losses.get_doa_loss(config.doa_loss)
    metric_class = _metrics.SELDMetrics(doa_threshold=config.lad_doa_thresh, n_classes=n_classes)
    model_path = os.path.join('./saved_model', config.name)
    os.makedirs(model_path, exist_ok=True)
    if getattr(config, 'resume', False):                           # train.py:322-331: the saved model's weights, not the optimizer's slots
        from glob import glob
        saved = sorted(glob(os.path.join(model_path, '*.npz')))
        if len(saved) == 0:
            raise ValueError('the model is not existing, resume fail')
        model.load_weights(saved[0])
    best, early, lr_pat, history = 99999.0, 0, 0, []
    for epoch in range(config.epoch if max_epochs is None else min(config.epoch, max_epochs)):
        if use_tdm and config.tdm_epoch != 0 and epoch % config.tdm_epoch == 0:      # train.py:341-356
            if epoch % 2 == 0 and epoch > 20:
                if overlap_sec < max_overlap_sec:
                    overlap_sec += 1
                elif overlap_num < max_overlap_num:
                    overlap_sec = 1
                    overlap_num += 1
                print(f'current_max_overlap_sec: {overlap_sec}, current_max_overlap_num: {overlap_num}')
            if not tdm_fresh:
                trainset = tdm_set()
            tdm_fresh = False
        metric_class.reset_states()
        tr = iterloop(model, trainset, sed_loss, doa_loss, metric_class, config, optimizer, 'train')
        metric_class.reset_states()
        va = iterloop(model, valset, sed_loss, doa_loss, metric_class, config, mode='val')
        score = va[2]
        metric_class.reset_states()                                 # evaluation loop (train.py:367-369)
        te = iterloop(model, testset, sed_loss, doa_loss, metric_class, config, mode='test')
        history.append({'epoch': epoch, 'train': tr, 'val': va, 'test': te, 'score': score, 'lr': optimizer.learning_rate})
        print(f'epoch {epoch}: train sed/doa/seld {tr[0]:.4f}/{tr[1]:.5f}/{tr[2]:.4f}  val {va[0]:.4f}/{va[1]:.5f}/{va[2]:.4f}'
              f'  test {te[0]:.4f}/{te[1]:.5f}/{te[2]:.4f}')
        if best > score:                                            # train.py:372-380
            old = os.path.join(model_path, f'bestscore_{best}.npz')
            if os.path.exists(old):
                os.remove(old)
            best, early, lr_pat = score, 0, 0
            model.save_weights(os.path.join(model_path, f'bestscore_{best}.npz'))
        else:                                                       # train.py:381-390
            if lr_pat == config.lr_patience and config.decay != 1:
                optimizer.learning_rate *= config.decay
                lr_pat = 0
            if early == config.patience:
                print(f'Early Stopping at {epoch}, score is {score}')
                break
            early += 1
            lr_pat += 1
    return model, history


if __name__ == '__main__':
    from . import params
    main(params.get_param())
