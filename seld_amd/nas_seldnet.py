"""The architecture search of the SELD task under the reference's names (nas_seldnet.py, config_sampler.py:23-89): configurations of
models.conv_temporal are drawn from a 2-D and a 1-D search space — the body's blocks and, from the 1-D space, a SED and a DOA head —
rewritten into buildable ones, filtered by a complexity window, trained for one pass and recorded in a JSON file a later run resumes.
Model, data, augmentation and metrics run on the device (modules.ConvTemporalNet with search=True: GRU stages of every width the space
offers on seld_rnn_gruw_*, attention stages of every key_dim on seld_attnw_*, simple_dense_stage's Dropout on the library's draws); there
is no CPU or PyTorch fallback.

  search_space_2d, search_space_1d        the reference's tables (nas_seldnet.py:37-77), value for value; the kinds it comments out stay out
  search_space_1d_attention               the two 1-D kinds the reference carries commented out (nas_seldnet.py:59-64, 70-76), value for value:
                                          transformer_encoder_stage and conformer_encoder_stage — the kinds the shipped SS5 model is made of;
                                          --attention_stages searches {**search_space_1d, **search_space_1d_attention}
  conv_temporal_sampler(space_2d, space_1d, n_blocks, input_shape, default_config, config_postprocess_fn, constraint, rng, max_tries)
                                          config_sampler.py:23-89: n_2d blocks from the 2-D space, then 1-D ones, SED and DOA from the 1-D
                                          space, each argument drawn uniformly; n_2d is drawn anew every 10,000 rejected configurations
  search_space_sanity_check, postprocess_fn   nas_vad's (the reference's two files hold the same text)
  sample_constraint(min_flops, max_flops, min_params, max_params)(model_config, input_shape)
                                          nas_seldnet.py:80-137: False for what cannot be built (ValueError from the plan on torch's meta
                                          device), for the degenerate mother_stages and outside the complexity window
  train_and_eval(train_config, model_config, input_shape, trainset, testset)   nas_seldnet.py:169-205: one pass with Adam(lr), BCE + MSE
                                          weighted (1, 1000), then SELDMetrics(doa_threshold=20) over the test set
  get_dataset(config, mode, device)       nas_seldnet.py:208-234: time mask 24, frequency mask 16, foa_intensity_vec_aug in training
  main(argv)                              nas_seldnet.py:237-291:  python -m seld_amd.nas_seldnet --name x --dataset_path DATA/feat_label

Deviations: `rng` (a numpy Generator, --seed) replaces the process-wide `random`; the complexity is ConvTemporalNet.complexity() — our own
count of the plan's products, not the reference's stage_complexity formulas, so the reference's 400M .. 480M window selects other
architectures than it does there; input_shape carries the batch in front ([B, T, F, C]; a 3-entry shape gets B = 1) and main reads T, F,
C off the data set where the reference hard-codes [300, 64, 7]; --label_window_size, --time_mask_size, --freq_mask_size (defaults 60, 24,
16: the reference's constants) are arguments, and the masks' period is the whole clip where 100 does not divide it; max_tries; the
history holds the mean loss and val_loss (the weighted sums) rather than Keras' per-output entries; --lr is a float; --attention_stages
(above) — of what search_space_1d_attention offers, a conformer kernel_size above 64 (the depthwise kernels end there), pos_encoding 'rff'
(its frequencies are drawn and stored nowhere) and 'basic' on an odd width (the reference's table does not broadcast) have no kernel: the
plan raises ValueError and sample_constraint answers False, so such a draw is rejected and drawn again, never built as something else."""
from __future__ import annotations

import argparse
import copy
import json
import os
import time

import numpy as np
import torch

from .nas_vad import RESAMPLE_EVERY, _block_keys, _pick, _with_batch, postprocess_fn, search_space_sanity_check  # noqa: F401

FILTERS = [0] * 11 + [3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256]
UNITS = [4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256]
search_space_2d = {
    "mother_stage": {
        "depth": [1, 2, 3],
        "filters0": list(FILTERS), "filters1": list(FILTERS), "filters2": list(FILTERS),
        "kernel_size0": [1, 3, 5], "kernel_size1": [1, 3, 5], "kernel_size2": [1, 3, 5],
        "connect0": [[0], [1]],
        "connect1": [[0, 0], [0, 1], [1, 0], [1, 1]],
        "connect2": [[a, b, c] for a in (0, 1) for b in (0, 1) for c in (0, 1)],
        "strides": [(1, 1), (1, 2), (1, 3)],
    },
}
search_space_1d = {
    "bidirectional_GRU_stage": {
        "depth": [1, 2, 3],
        "units": list(UNITS),
    },
    "simple_dense_stage": {
        "depth": [1, 2, 3],
        "units": list(UNITS),
        "dense_activation": ["relu"],
        "dropout_rate": [0., 0.2, 0.5],
    },
}
KEY_DIMS = [2, 3, 4, 6, 8, 12, 16, 24, 32, 48]
search_space_1d_attention = {
    "transformer_encoder_stage": {
        "depth": [1, 2, 3],
        "n_head": [1, 2, 4, 8, 16],
        "key_dim": list(KEY_DIMS),
        "ff_multiplier": [0.25, 0.5, 1, 2, 4, 8],
        "kernel_size": [1, 3, 5],
    },
    "conformer_encoder_stage": {
        "depth": [1, 2, 3],
        "key_dim": list(KEY_DIMS),
        "n_head": [1, 2, 4, 8, 16],
        "kernel_size": [4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256],
        "multiplier": [1, 2, 4],
        "pos_encoding": [None, "basic", "rff"],
    },
}
LOSS_WEIGHTS = (1.0, 1000.0)      # nas_seldnet.py:181
DOA_THRESHOLD = 20                # nas_seldnet.py:250


def conv_temporal_sampler(search_space_2d: dict, search_space_1d: dict, n_blocks: int, input_shape, default_config=None,
                          config_postprocess_fn=None, constraint=None, rng=None, max_tries=None):
    """-> a model_config the constraint accepts.  max_tries (ours): give up with a RuntimeError instead of drawing for ever"""
    search_space_sanity_check(search_space_2d)
    search_space_sanity_check(search_space_1d)
    rng = rng or np.random.default_rng()
    total = {**search_space_2d, **search_space_1d}
    names_2d, names_1d = list(search_space_2d), list(search_space_1d)
    count = 0
    while max_tries is None or count < max_tries:
        if count % RESAMPLE_EVERY == 0:
            n_2d = n_blocks if not names_1d else int(rng.integers(0, n_blocks + 1))
            if count:
                print(f"{count}th iters. check constraint")
        count += 1
        model_config = copy.deepcopy(default_config or {})
        for i in range(n_blocks):
            module = _pick(rng, names_2d if i < n_2d else names_1d)
            model_config[f"BLOCK{i}"] = module
            model_config[f"BLOCK{i}_ARGS"] = {k: _pick(rng, v) for k, v in total[module].items()}
        for head in ("SED", "DOA"):      # the heads only take 1-D modules
            module = _pick(rng, names_1d)
            model_config[head] = module
            model_config[f"{head}_ARGS"] = {k: _pick(rng, v) for k, v in total[module].items()}
        if config_postprocess_fn is not None:
            model_config = config_postprocess_fn(model_config)
        if constraint is None or constraint(model_config, input_shape):
            return model_config
    raise RuntimeError(f"conv_temporal_sampler: no configuration passed the constraint in {max_tries} draws")


def plan(model_config: dict, input_shape):
    """the model's plan on torch's meta device: shapes and variables, nothing allocated"""
    from .modules import ConvTemporalNet
    return ConvTemporalNet(_with_batch(input_shape), model_config, device="meta", search=True)


def sample_constraint(min_flops=None, max_flops=None, min_params=None, max_params=None):
    def _constraint(model_config, input_shape):
        for key in _block_keys(model_config):
            if model_config[key] != "mother_stage":
                continue
            a = model_config[f"{key}_ARGS"]
            n_convs = sum(int(a[f"filters{i}"] > 0) for i in range(3))
            if n_convs == 1 and a["filters1"] == 0:
                return False      # one convolution that is not the strided one
            if n_convs == 2 and a["filters1"] > 0 and [int(v) for v in a["strides"]] == [1, 1]:
                return False
        try:
            cx = plan(model_config, input_shape).complexity()
        except ValueError:
            return False
        for lo, hi, k in ((min_flops, max_flops, "flops"), (min_params, max_params, "params")):
            if (lo and cx[k] < lo) or (hi and cx[k] > hi):
                return False
        return True
    return _constraint


def _device_batch(dataset, x, y, dev):
    """a batch of `dataset` on the device, augmented by its device transforms -> x, (y_sed, y_doa)  (train.iterloop's first lines)"""
    dev_tf = getattr(dataset, "device_transforms", None)
    if not dev_tf:
        return x, y
    x = torch.as_tensor(x, dtype=torch.float32).to(dev).contiguous()
    y = torch.as_tensor(y, dtype=torch.float32).to(dev).contiguous()
    for f in dev_tf:
        x, y = f(x, y, dataset.rng)
    nc = y.shape[-1] // 4
    return x, (y[..., :nc].contiguous(), y[..., nc:].contiguous())


def train_and_eval(train_config, model_config: dict, input_shape, trainset, testset) -> dict:
    """one pass over trainset with Adam(train_config.lr), one over testset -> the history (one entry per figure), the SELD scores of the
    test set and the complexity"""
    from . import losses, metrics, models
    from .train import Adam, teststep, trainstep
    model = models.conv_temporal(_with_batch(input_shape), model_config, search=True)
    optimizer = Adam(float(train_config.lr))
    sed_loss, doa_loss = losses.BinaryCrossentropy(), losses.MSE
    evaluator = metrics.SELDMetrics(doa_threshold=DOA_THRESHOLD, n_classes=model.n_classes, device=model._dev.index)
    sums = torch.zeros(2, dtype=torch.float32, device=model._dev)
    steps = [0, 0]
    for x, y in trainset:
        x, y = _device_batch(trainset, x, y, model._dev)
        _, sloss, dloss = trainstep(model, x, y, sed_loss, doa_loss, LOSS_WEIGHTS, optimizer)
        sums[0] += LOSS_WEIGHTS[0] * sloss + LOSS_WEIGHTS[1] * dloss.mean()
        steps[0] += 1
    for x, y in testset:
        x, y = _device_batch(testset, x, y, model._dev)
        preds, sloss, dloss = teststep(model, x, y, sed_loss, doa_loss)
        evaluator.update_states(y, preds)
        sums[1] += LOSS_WEIGHTS[0] * sloss + LOSS_WEIGHTS[1] * dloss.mean()
        steps[1] += 1
    scores = evaluator.result()      # the one synchronisation
    tot = sums.tolist()
    out = {"loss": [tot[0] / max(steps[0], 1)], "val_loss": [tot[1] / max(steps[1], 1)],
           "test_error_rate": scores[0], "test_f1score": scores[1], "test_der": scores[2], "test_derf": scores[3],
           "test_seld_score": float(metrics.calculate_seld_score(scores))}
    out.update(model.complexity())
    model.close()
    return out


def get_dataset(config, mode: str = "train", device=None):
    """the windowed data set of `mode` ('train': folds 1-4, 'test': fold 6) under config.dataset_path; training: a time mask up to 24 frames
    and a frequency mask up to 16 bins per sample, then foa_intensity_vec_aug on the batch, config.n_repeat passes — all on the device"""
    from . import data_loader as dl
    from . import transforms as tfm
    path = config.dataset_path
    x, y = dl.load_seldnet_data(os.path.join(path, "foa_dev_norm"), os.path.join(path, "foa_dev_label"), mode=mode, n_freq_bins=64)
    if not x:
        raise ValueError(f"{path}: no {mode} clips")
    device_transforms = []
    if mode == "train":
        tmask, fmask = int(getattr(config, "time_mask_size", 24)), int(getattr(config, "freq_mask_size", 16))

        def masks(xb, yb, rng):
            T = xb.shape[1]
            period = 100 if T % 100 == 0 else T
            tfm.mask(xb, -3, max_mask_size=tmask, period=period, rng=rng)
            tfm.mask(xb, -2, max_mask_size=fmask, period=period, rng=rng)
            return xb, yb
        device_transforms = [masks, lambda xb, yb, rng: tfm.foa_intensity_vec_aug(xb, yb, rng=rng)]
    ds = dl.seldnet_data_to_dataloader(x, y, train=mode == "train", label_window_size=int(getattr(config, "label_window_size", 60)),
                                       batch_size=config.batch_size, loop_time=config.n_repeat, seed=getattr(config, "seed", None),
                                       device_transforms=device_transforms)
    return ds.to_device(device) if device is not None else ds


def get_parser():
    args = argparse.ArgumentParser()
    args.add_argument("--name", type=str, required=True, help="the results go to {name}.json")
    args.add_argument("--dataset_path", type=str, default="/root/datasets/DCASE2021/feat_label")
    args.add_argument("--n_samples", type=int, default=256)
    args.add_argument("--n_blocks", type=int, default=4)
    args.add_argument("--min_flops", type=int, default=400_000_000)
    args.add_argument("--max_flops", type=int, default=480_000_000)
    args.add_argument("--batch_size", type=int, default=256)
    args.add_argument("--n_repeat", type=int, default=50)
    args.add_argument("--lr", type=float, default=1e-3)
    args.add_argument("--n_classes", type=int, default=12)
    args.add_argument("--label_window_size", type=int, default=60)
    args.add_argument("--time_mask_size", type=int, default=24)
    args.add_argument("--freq_mask_size", type=int, default=16)
    args.add_argument("--seed", type=int, default=0)
    args.add_argument("--attention_stages", action="store_true",
                      help="also draw transformer_encoder_stage / conformer_encoder_stage (search_space_1d_attention)")
    return args


def main(argv=None) -> dict:
    train_config = get_parser().parse_args(argv)
    name = train_config.name if train_config.name.endswith(".json") else f"{train_config.name}.json"
    results = {"train_config": vars(train_config)}
    start_idx = 0
    if os.path.exists(name):      # resume past results; checked before anything touches the data or a device
        with open(name) as f:
            prev = json.load(f)
        prev["train_config"].setdefault("attention_stages", False)      # a file from before the option existed
        if results["train_config"] != prev["train_config"]:
            raise ValueError("prev config has different train_config")
        results = prev
        start_idx = 1 + max([int(k) for k in results if k.isdigit()], default=-1)
    dev = torch.cuda.current_device() if torch.cuda.is_available() else None
    trainset = get_dataset(train_config, "train", dev)
    testset = get_dataset(train_config, "test", dev)
    n_windows = max(int(train_config.batch_size), int(testset.batch_size))
    input_shape = [n_windows] + [int(v) for v in trainset.x.shape[1:]]
    default_config = {"n_classes": train_config.n_classes}
    constraint = sample_constraint(train_config.min_flops, train_config.max_flops)
    rng = np.random.default_rng([train_config.seed, start_idx])
    space_1d = {**search_space_1d, **search_space_1d_attention} if train_config.attention_stages else search_space_1d
    for i in range(start_idx, train_config.n_samples):
        model_config = conv_temporal_sampler(search_space_2d, space_1d, n_blocks=train_config.n_blocks, input_shape=input_shape,
                                             default_config=default_config, config_postprocess_fn=postprocess_fn, constraint=constraint, rng=rng)
        start = time.time()
        outputs = train_and_eval(train_config, model_config, input_shape, trainset, testset)
        outputs["time"] = time.time() - start
        results[f"{i:03d}"] = {"config": model_config, "perf": outputs}
        with open(name, "w") as f:
            json.dump(results, f, indent=4)
    return results


if __name__ == "__main__":
    main()
