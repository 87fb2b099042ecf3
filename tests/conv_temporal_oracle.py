"""fp64 restatement (torch, CPU) of the reference's models.conv_temporal (models.py:54-78) with every Dropout at rate 0, composed from the
oracles of its parts.  A helper, not a test file: tests/test_conv_temporal_cpu.py pins its own pieces, tests/test_conv_temporal_gpu.py checks
the device against it.

  maxpool2d              MaxPooling2D(pool, strides = pool, 'same' | 'valid') on NHWC.  TensorFlow 'SAME': out = ceil(n / p), pad_total =
                         out p - n, pad_before = pad_total // 2 and the surplus behind — F.pad with -inf by exactly (before, after), then
                         max_pool2d WITHOUT padding (torch's own padding is symmetric and does not match TensorFlow)
  stem                   layers.conv2d_bn(filters, k, 'same', relu) (layers.py:14-38) + MaxPooling2D(first_pool_size, 'same')
  chain                  the BLOCK* keys sorted as strings (models.py:66-68); mother_block / mother_stage (oracle.modules_oracle); the stage
                         wrappers as the reference writes them (modules.py:46-61, 86-103): bidirectional_GRU_stage = depth x [units],
                         simple_dense_stage = depth x [units] with dense_activation = model_config.get('activation') — overwriting
                         whatever dense_activation the configuration holds; the 3-D kinds of tests/transformer_oracle.py,
                         tests/conformer_oracle.py, tests/attention_block_oracle.py, tests/rnn_oracle.py
  heads                  SED / DOA: a 3-D kind, then Dense(n_classes, sigmoid) / Dense(3 n_classes, tanh)
"""
from __future__ import annotations

import copy
from typing import Dict

import numpy as np
import torch
import torch.nn.functional as F

import attention_block_oracle as A
import conformer_oracle as K
import rnn_oracle as R
import transformer_oracle as T
from oracle import modules_oracle as M
from oracle import seldnet_oracle as O

ACTS = T.ACTS
f32 = T.f32


# ---------------------------------------------------------------- pooling
def same_pads(n: int, p: int):
    """-> (out, pad_before, pad_after) of TensorFlow 'SAME' with strides == pool"""
    out = -(-n // p)
    tot = out * p - n
    return out, tot // 2, tot - tot // 2


def maxpool2d(x, pool, padding: str = "same"):
    """x [B, H, W, C] -> [B, Ho, Wo, C]"""
    ph, pw = pool
    t = x.permute(0, 3, 1, 2)
    if padding == "same":
        _, hb, ha = same_pads(x.shape[1], ph)
        _, wb, wa = same_pads(x.shape[2], pw)
        t = F.pad(t, (wb, wa, hb, ha), value=float("-inf"))
    return F.max_pool2d(t, (ph, pw), stride=(ph, pw), padding=0).permute(0, 2, 3, 1)


def pool_windows(x, pool, padding: str = "same"):
    """x [B, H, W, C] -> [B, Ho, Wo, ph * pw, C]: every window's elements in row-major window order, -inf where the window leaves the tensor"""
    ph, pw = pool
    t = x.permute(0, 3, 1, 2)
    if padding == "same":
        _, hb, ha = same_pads(x.shape[1], ph)
        _, wb, wa = same_pads(x.shape[2], pw)
        t = F.pad(t, (wb, wa, hb, ha), value=float("-inf"))
    Ho, Wo = t.shape[2] // ph, t.shape[3] // pw
    t = t[:, :, :Ho * ph, :Wo * pw].reshape(t.shape[0], t.shape[1], Ho, ph, Wo, pw)
    return t.permute(0, 2, 4, 3, 5, 1).reshape(t.shape[0], Ho, Wo, ph * pw, t.shape[1])


# ---------------------------------------------------------------- the chain
def blocks_of(model_config: dict):
    keys = [k for k in model_config.keys() if k.startswith("BLOCK") and not k.endswith("_ARGS")]
    keys.sort()
    return keys


def _wrap(kind: str, args: dict):
    """the reference's stage wrappers and identity_block as the blocks they build"""
    a = copy.deepcopy(args)
    if kind == "bidirectional_GRU_stage":      # modules.py:46-61
        a["units"] = [a["units"]] * a["depth"]
        return "bidirectional_GRU_block", a
    if kind == "simple_dense_stage":           # modules.py:86-103
        a["units"] = [a["units"]] * a["depth"]
        a["dense_activation"] = a.get("activation", None)
        return "simple_dense_block", a
    if kind == "identity_block":               # modules.py:639-642
        return "simple_dense_block", {"units": []}
    return kind, a


STAGED = {"transformer_encoder_block": (T, "tf", False), "transformer_encoder_stage": (T, "tf", True),
          "conformer_encoder_block": (K, "cf", False), "conformer_encoder_stage": (K, "cf", True),
          "attention_block": (A, "at", False), "attention_stage": (A, "at", True),
          "RNN_block": (R, "rnn", False), "RNN_stage": (R, "rnn", True)}


def _specs_3d(kind: str, args: dict, D: int, prefix: str):
    """-> (trainable, state, out_dim)"""
    kind, a = _wrap(kind, args)
    if kind == "simple_dense_block":
        tr, k = [], int(a.get("kernel_size", 1))
        for j, u in enumerate(a["units"]):
            tr += [(f"{prefix}.dense{j}.kernel", (k, D, int(u))), (f"{prefix}.dense{j}.bias", (int(u),))]
            D = int(u)
        return tr, [], D
    if kind == "bidirectional_GRU_block":
        tr = []
        for i, u in enumerate(a["units"]):
            tr += R.block_specs(D, {"units": int(u)}, f"{prefix}.gru{i}")
            D = int(u)
        return tr, [], D
    mod, pre, stage = STAGED[kind]
    depth = int(a["depth"]) if stage else 1
    sp = mod.stage_specs(D, a, depth, f"{prefix}.{pre}")
    tr, nt = sp if isinstance(sp, tuple) else (sp, [])
    return tr, nt, (R.out_dim(a) if mod is R else D)


def _forward_3d(kind: str, args: dict, x, w, st, new_st, training: bool, prefix: str):
    """x [B, S, D] -> [B, S, out_dim]"""
    kind, a = _wrap(kind, args)
    if kind == "simple_dense_block":
        act = ACTS[a.get("dense_activation", None)]
        for j in range(len(a["units"])):
            x = act(O.conv1d_same(x, w[f"{prefix}.dense{j}.kernel"], w[f"{prefix}.dense{j}.bias"]))
        return x
    if kind == "bidirectional_GRU_block":
        for i in range(len(a["units"])):
            x = O.bigru_mul(x, w, f"{prefix}.gru{i}")
        return x
    mod, pre, stage = STAGED[kind]
    depth = int(a["depth"]) if stage else 1
    if mod in (T, R):
        return mod.stage_forward(x, w, a, depth, f"{prefix}.{pre}")
    return mod.stage_forward(x, w, st, new_st, a, depth, training, f"{prefix}.{pre}")


def _mother_cfgs(kind: str, args: dict):
    return M.stage_configs(args) if kind == "mother_stage" else [copy.deepcopy(args)]


def stem_out(model_config: dict, input_shape):
    T_, Fq, _ = (int(v) for v in input_shape[-3:])
    ph, pw = model_config.get("first_pool_size", [5, 1])
    return (same_pads(T_, ph)[0], same_pads(Fq, pw)[0], int(model_config.get("filters", 32)))


def variable_specs(model_config: dict, input_shape):
    """-> (trainable, state) [(name, shape)] in the reference's creation order"""
    Cin = int(input_shape[-1])
    Fl, k = int(model_config.get("filters", 32)), int(model_config.get("first_kernel_size", 7))
    nc = int(model_config.get("n_classes", 14))
    tr = [("stem.conv.kernel", (k, k, Cin, Fl)), ("stem.conv.bias", (Fl,)), ("stem.bn.gamma", (Fl,)), ("stem.bn.beta", (Fl,))]
    nt = [("stem.bn.moving_mean", (Fl,)), ("stem.bn.moving_variance", (Fl,))]
    shape, D = stem_out(model_config, input_shape), None
    for i, key in enumerate(blocks_of(model_config)):
        kind, args = model_config[key], model_config[f"{key}_ARGS"]
        if kind in ("mother_block", "mother_stage"):
            assert D is None
            for d, c in enumerate(_mother_cfgs(kind, args)):
                t, n, shape = M.mother_block_plan(c, shape, f"b{i}.mb{d}")
                tr += t
                nt += n
        else:
            D = shape[1] * shape[2] if D is None else D
            t, n, D = _specs_3d(kind, args, D, f"b{i}")
            tr += t
            nt += n
    D = shape[1] * shape[2] if D is None else D
    for head, n_out in (("sed", nc), ("doa", 3 * nc)):
        t, n, Dh = _specs_3d(model_config[head.upper()], model_config.get(f"{head.upper()}_ARGS", {}), D, head)
        tr += t + [(f"{head}_out.kernel", (Dh, n_out)), (f"{head}_out.bias", (n_out,))]
        nt += n
    return tr, nt


def random_weights(model_config: dict, input_shape, seed: int = 0):
    """T.random_block_weights' rules (glorot-uniform kernels, every bias / gamma / beta perturbed); moving statistics away from 0 / 1"""
    tr, nt = variable_specs(model_config, input_shape)
    rng = np.random.default_rng(seed + 7)
    st = [0.1 * rng.standard_normal(int(np.prod(s))) if n.endswith("moving_mean") else 1.0 + 0.3 * rng.random(int(np.prod(s))) for n, s in nt]
    return T.random_block_weights(tr, seed), np.concatenate(st).astype(np.float32)


def forward(model_config: dict, w: Dict[str, torch.Tensor], st: Dict[str, torch.Tensor], x, training: bool):
    """-> (sed, doa, new_state)"""
    new_st = dict(st)
    z = M.conv2d_same(x, w["stem.conv.kernel"], w["stem.conv.bias"])
    y, m, v = O.batchnorm(z, w["stem.bn.gamma"], w["stem.bn.beta"], st["stem.bn.moving_mean"], st["stem.bn.moving_variance"], training)
    new_st["stem.bn.moving_mean"], new_st["stem.bn.moving_variance"] = m, v
    h = maxpool2d(torch.relu(y), tuple(model_config.get("first_pool_size", [5, 1])), "same")
    for i, key in enumerate(blocks_of(model_config)):
        kind, args = model_config[key], model_config[f"{key}_ARGS"]
        if kind in ("mother_block", "mother_stage"):
            for d, c in enumerate(_mother_cfgs(kind, args)):
                h = M.mother_block_forward(c, w, st, new_st, h, training, f"b{i}.mb{d}")
        else:
            if h.dim() == 4:
                h = h.reshape(h.shape[0], h.shape[1], -1)      # layers.force_1d_inputs (layers.py:41-47)
            h = _forward_3d(kind, args, h, w, st, new_st, training, f"b{i}")
    if h.dim() == 4:
        h = h.reshape(h.shape[0], h.shape[1], -1)
    outs = []
    for head, act in (("sed", torch.sigmoid), ("doa", torch.tanh)):
        a = _forward_3d(model_config[head.upper()], model_config.get(f"{head.upper()}_ARGS", {}), h, w, st, new_st, training, head)
        outs.append(act(a @ w[f"{head}_out.kernel"] + w[f"{head}_out.bias"]))
    return outs[0], outs[1], new_st


def train_step(model_config: dict, input_shape, flat_w, flat_state, x, y_sed, y_doa, *, doa_loss="MSE", loss_weight=(1.0, 1000.0), lr=1e-3,
               step=1, dtype=torch.float64):
    """train.trainstep (train.py:22-36) -> dict(sed, doa, sloss, dloss, grad, new_w, new_state), all numpy"""
    tr, nt = variable_specs(model_config, input_shape)
    fw = torch.tensor(np.asarray(flat_w), dtype=dtype, requires_grad=True)
    wd = O.unflatten(fw, tr)
    sd = O.unflatten(torch.tensor(np.asarray(flat_state), dtype=dtype), nt)
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype)
    sed, doa, new_st = forward(model_config, wd, sd, t(x), True)
    obj, sloss, dloss = O.losses_and_objective(sed, doa, t(y_sed), t(y_doa), doa_loss, loss_weight)
    (g,) = torch.autograd.grad(obj, fw)
    new_w, _, _ = O.adam_update(fw.detach(), g, torch.zeros_like(fw), torch.zeros_like(fw), step, lr=lr)
    ns = torch.cat([new_st[n].detach().reshape(-1) for n, _ in nt])
    return {"sed": sed.detach().numpy(), "doa": doa.detach().numpy(), "sloss": sloss.detach().numpy(), "dloss": dloss.detach().numpy(),
            "grad": g.numpy(), "new_w": new_w.numpy(), "new_state": ns.numpy()}


def inference(model_config: dict, input_shape, flat_w, flat_state, x, dtype=torch.float64):
    """-> (sed, doa) numpy"""
    tr, nt = variable_specs(model_config, input_shape)
    wd = O.unflatten(torch.tensor(np.asarray(flat_w), dtype=dtype), tr)
    sd = O.unflatten(torch.tensor(np.asarray(flat_state), dtype=dtype), nt)
    with torch.no_grad():
        sed, doa, _ = forward(model_config, wd, sd, torch.as_tensor(np.asarray(x), dtype=dtype), False)
    return sed.numpy(), doa.numpy()


# ---------------------------------------------------------------- the configurations of the tests
MOTHER = {"filters0": 0, "filters1": 96, "filters2": 0, "kernel_size0": 0, "kernel_size1": 3, "kernel_size2": 0, "connect0": [1],
          "connect1": [1, 0], "connect2": [1, 0, 1], "strides": [1, 3]}      # SS5.json's BLOCK0_ARGS without `depth`

# SS5.json's shape at a small input, every Dropout at 0: mother_stage, simple_dense_stage (its dense_activation 'relu' is overwritten by the
# absent `activation`: a linear layer), two conformer blocks; a conformer stage as the SED head, a bidirectional_GRU_stage as the DOA head
SS5_SMALL = {
    "n_classes": 12, "first_pool_size": [5, 2],
    "BLOCK0": "mother_stage", "BLOCK0_ARGS": dict(MOTHER, depth=2, filters1=24),
    "BLOCK1": "simple_dense_stage", "BLOCK1_ARGS": {"depth": 1, "units": 96, "dense_activation": "relu", "dropout_rate": 0.0},
    "BLOCK2": "conformer_encoder_stage",
    "BLOCK2_ARGS": {"depth": 2, "key_dim": 24, "n_head": 4, "kernel_size": 24, "multiplier": 2, "pos_encoding": None, "dropout_rate": 0},
    "SED": "conformer_encoder_stage",
    "SED_ARGS": {"depth": 1, "key_dim": 48, "n_head": 4, "kernel_size": 8, "multiplier": 2, "pos_encoding": None, "dropout_rate": 0},
    "DOA": "bidirectional_GRU_stage", "DOA_ARGS": {"depth": 2, "units": 128},
}
SS5_SMALL_INPUT = (2, 52, 15, 7)

# a second chain: mother_block -> RNN_stage (LSTM, concat) -> transformer_encoder_block; SED identity_block, DOA simple_dense_stage
CHAIN2 = {
    "n_classes": 5, "filters": 8, "first_kernel_size": 3, "first_pool_size": [2, 3],
    "BLOCK0": "mother_block",
    "BLOCK0_ARGS": {"filters0": 6, "filters1": 0, "filters2": 12, "kernel_size0": 3, "kernel_size1": 0, "kernel_size2": 1, "connect0": [1],
                    "connect1": [0, 1], "connect2": [1, 1, 0]},
    "BLOCK1": "RNN_stage", "BLOCK1_ARGS": {"depth": 1, "units": 128, "rnn_type": "LSTM", "merge_mode": "concat"},
    "BLOCK2": "transformer_encoder_block",
    "BLOCK2_ARGS": {"n_head": 2, "key_dim": 16, "ff_multiplier": 0.5, "kernel_size": 3, "dropout_rate": 0},
    "SED": "identity_block", "SED_ARGS": {},
    "DOA": "simple_dense_stage", "DOA_ARGS": {"depth": 2, "units": 24, "activation": "tanh"},
}
CHAIN2_INPUT = (3, 15, 10, 4)


def synthetic_batch(model_config: dict, input_shape, seed: int = 5):
    """-> (x, y_sed, y_doa): x ~ N(0.3, 1) (a mean the stem's BatchNormalization has to remove), labels as O.synthetic_batch draws them"""
    B, T_, Fq, Ch = input_shape
    nc = int(model_config.get("n_classes", 14))
    S = stem_out(model_config, input_shape)[0]
    _, ys, yd = O.synthetic_batch(B, 5 * S, Fq, Ch, n_classes=nc, seed=seed)
    rng = np.random.default_rng(seed)
    return f32(0.3 + rng.standard_normal((B, T_, Fq, Ch))), ys, yd
