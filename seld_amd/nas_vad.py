"""The architecture search of the voice-activity task under the reference's names (nas_vad.py, config_sampler.py:92-147): configurations of
models.vad_architecture are drawn from a 2-D and a 1-D search space, rewritten into buildable ones, filtered by a complexity window, trained
for one pass and recorded in a JSON file a later run resumes.  Models, data and metrics run on the device (seld_amd/modules.py VadArchNet,
vad_dataloader.py, vad_metrics.py); there is no CPU or PyTorch fallback.

  search_space_2d, search_space_1d        the reference's tables (nas_vad.py:44-68), value for value
  search_space_sanity_check(space)        config_sampler.py:140-147: every value of every block is a non-empty list or tuple
  vad_architecture_sampler(space_2d, space_1d, n_blocks, input_shape, default_config, config_postprocess_fn, constraint, rng)
                                          config_sampler.py:92-137: n_2d blocks from the 2-D space, then 1-D ones, each argument drawn
                                          uniformly; n_2d is drawn anew every 10,000 rejected configurations
  postprocess_fn(model_config)            nas_vad.py:123-149: a mother_stage's skipped layers get kernel size 0 and lose their links
  sample_constraint(min_flops, max_flops, min_params, max_params)(model_config, input_shape)
                                          nas_vad.py:71-120: False for what cannot be built (ValueError from the plan on torch's meta device),
                                          for the degenerate mother_stages the reference excludes and outside the complexity window
  train_and_eval(train_config, model_config, input_shape, trainset, testset)   nas_vad.py:164-185: one pass with Adam(lr), one validation pass
  main(argv)                              nas_vad.py:188-242

Deviations: `rng` (a numpy Generator) replaces the process-wide `random`; the complexity is VadArchNet.complexity() — our own count of the
plan's dense products, not the reference's stage_complexity formulas, so the reference's 500,000 .. 600,000 window selects other
architectures than it does there; input_shape carries the batch in front ([B, Wn, F, C]; a 3-entry shape gets B = 1); the data sets are
.npz pair lists (--train, --test: arrays x0, y0, x1, y1, ... = features [frames, F, C] and frame labels [frames]) where the reference
hard-codes two joblib files, and the window is an argument; a resumed run may ask for more samples (n_samples is not compared); the
history holds loss, val_loss and the val_* figures of VADMetrics."""
from __future__ import annotations

import argparse
import copy
import json
import os
import time

import numpy as np
import torch

FILTERS = [0] * 11 + [3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256]
UNITS = [3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256]
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
    "simple_dense_stage": {
        "depth": [1, 2, 3],
        "units": list(UNITS),
        "dense_activation": [None, "relu"],
        "dropout_rate": [0., 0.2, 0.5],
    },
}
REF_WINDOW = [-19, -10, -1, 0, 1, 10, 19]      # nas_vad.py:191
RESAMPLE_EVERY = 10000


def _block_keys(model_config: dict):
    from .modules import chain_blocks
    return chain_blocks(model_config)


def search_space_sanity_check(search_space: dict) -> None:
    for name, space in search_space.items():
        for v in space.values():
            if not isinstance(v, (list, tuple)):
                raise ValueError(f"values of {name} must be tuple or list")
            if len(v) == 0:
                raise ValueError(f"len of value in {name} must be > 0")


def _pick(rng, seq):
    seq = list(seq)
    return copy.deepcopy(seq[int(rng.integers(len(seq)))])


def vad_architecture_sampler(search_space_2d: dict, search_space_1d: dict, n_blocks: int, input_shape, default_config=None,
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
        if config_postprocess_fn is not None:
            model_config = config_postprocess_fn(model_config)
        if constraint is None or constraint(model_config, input_shape):
            return model_config
    raise RuntimeError(f"vad_architecture_sampler: no configuration passed the constraint in {max_tries} draws")


def postprocess_fn(model_config: dict) -> dict:
    """a mother_stage whose last layer is skipped hands on the layer in front of it; a skipped layer has kernel size 0, nothing links to it,
    and without the second layer there are no strides"""
    model_config = copy.deepcopy(model_config)
    for key in _block_keys(model_config):
        if model_config[key] != "mother_stage":
            continue
        a = model_config[f"{key}_ARGS"]
        a["connect1"], a["connect2"] = list(a["connect1"]), list(a["connect2"])
        if a["filters2"] == 0:
            if a["filters1"] != 0:
                a["connect2"][2] = 1
            elif a["filters0"] != 0:
                a["connect2"][1] = 1
        if a["filters0"] == 0:
            a["kernel_size0"] = 0
            a["connect1"][1] = a["connect2"][1] = 0
        if a["filters1"] == 0:
            a["kernel_size1"] = 0
            a["connect2"][2] = 0
            a["strides"] = [1, 1]
        if a["filters2"] == 0:
            a["kernel_size2"] = 0
    return model_config


def _with_batch(input_shape):
    sh = [int(v) for v in input_shape]
    return sh if len(sh) == 4 else [1] + sh


def plan(model_config: dict, input_shape):
    """the model's plan on torch's meta device: shapes and variables, nothing allocated"""
    from .modules import VadArchNet
    return VadArchNet(_with_batch(input_shape), model_config, device="meta")


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


def train_and_eval(train_config, model_config: dict, input_shape, trainset, testset) -> dict:
    """one pass over trainset with Adam(train_config.lr), one over testset -> the history (one entry per figure) merged with the complexity"""
    from .modules import VadArchNet
    from .train import Adam
    from .vad_metrics import VADMetrics
    model = VadArchNet(_with_batch(input_shape), model_config)
    optimizer = Adam(float(train_config.lr))
    metrics = VADMetrics(device=model._dev.index)
    sums = torch.zeros(2, dtype=torch.float32, device=model._dev)
    steps = [0, 0]
    for x, y in trainset:
        sums[0] += model.train_step(x, y, optimizer)[1]
        steps[0] += 1
    for x, y in testset:
        p, loss = model.test_step(x, y)
        metrics.update_state(y, p)
        sums[1] += loss
        steps[1] += 1
    res = metrics.result()      # the one synchronisation
    tot = sums.tolist()
    out = {"loss": [tot[0] / max(steps[0], 1)], "val_loss": [tot[1] / max(steps[1], 1)]}
    out.update({f"val_{k}": [v] for k, v in res.items()})
    out.update(model.complexity())
    model.close()
    return out


def load_pairs(path):
    """an .npz pair list: x0, y0, x1, y1, ... -> [(features [frames, F, C], labels [frames])]"""
    z = np.load(path)
    n = len([k for k in z.files if k.startswith("x")])
    if n < 1 or any(f"{c}{i}" not in z.files for i in range(n) for c in "xy"):
        raise ValueError(f"{path}: arrays x0, y0, x1, y1, ...")
    return [(np.asarray(z[f"x{i}"], np.float32), np.asarray(z[f"y{i}"], np.float32)) for i in range(n)]


def get_parser():
    args = argparse.ArgumentParser()
    args.add_argument("--json_fname", type=str, default="vad_results.json")
    args.add_argument("--n_samples", type=int, default=256)
    args.add_argument("--n_blocks", type=int, default=3)
    args.add_argument("--min_flops", type=int, default=500_000)
    args.add_argument("--max_flops", type=int, default=600_000)
    args.add_argument("--batch_size", type=int, default=256)
    args.add_argument("--n_repeat", type=int, default=50)
    args.add_argument("--lr", type=float, default=1e-3)
    args.add_argument("--train", type=str, required=True, help=".npz pair list of the training utterances")
    args.add_argument("--test", type=str, required=True, help=".npz pair list of the test utterances")
    args.add_argument("--window", type=int, nargs="+", default=REF_WINDOW)
    args.add_argument("--seed", type=int, default=0)
    return args


def main(argv=None) -> dict:
    from .train_vad_baseline import prepare_dataset
    train_config = get_parser().parse_args(argv)
    train_pairs, test_pairs = load_pairs(train_config.train), load_pairs(train_config.test)
    window = list(train_config.window)
    input_shape = [train_config.batch_size, len(window)] + list(train_pairs[0][0].shape[1:])
    default_config = {"flatten": False, "last_unit": 1}
    constraint = sample_constraint(train_config.min_flops, train_config.max_flops)
    results = {"train_config": vars(train_config)}
    start_idx = 0
    if os.path.exists(train_config.json_fname):      # resume past results
        with open(train_config.json_fname) as f:
            prev = json.load(f)
        same = lambda c: {k: v for k, v in c.items() if k != "n_samples"}
        if same(results["train_config"]) != same(prev["train_config"]):
            raise ValueError("prev config has different train_config")
        prev["train_config"] = results["train_config"]
        results = prev
        start_idx = 1 + max([int(k) for k in results if k.isdigit()], default=-1)
    rng = np.random.default_rng([train_config.seed, start_idx])
    trainset = prepare_dataset(train_pairs, window, train_config.batch_size, train=True, n_repeat=train_config.n_repeat, rng=rng)
    testset = prepare_dataset(test_pairs, window, train_config.batch_size, train=False)
    for i in range(start_idx, train_config.n_samples):
        model_config = vad_architecture_sampler(search_space_2d, search_space_1d, n_blocks=train_config.n_blocks, input_shape=input_shape,
                                                default_config=default_config, config_postprocess_fn=postprocess_fn, constraint=constraint, rng=rng)
        start = time.time()
        outputs = train_and_eval(train_config, model_config, input_shape, trainset, testset)
        outputs["time"] = time.time() - start
        results[f"{i:03d}"] = {"config": model_config, "perf": outputs}
        with open(train_config.json_fname, "w") as f:
            json.dump(results, f, indent=4)
    return results


if __name__ == "__main__":
    main()
