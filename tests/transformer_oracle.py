"""fp64 restatement (torch, CPU) of what seld_amd/modules.py adds for the reference's transformer_encoder_block / _stage
(modules.py:106-126, 379-407).  A helper, not a test file: tests/test_attention_cpu.py pins it against torch's own operators, and
tests/test_attention_gpu.py checks the device against it.

  attention            tf.keras.layers.MultiHeadAttention's core (modules.py:392-393): softmax(scale Q K^T) V per head
  layer_norm           tf.keras.layers.LayerNormalization() (modules.py:395, 403): last axis, biased variance, eps = 1e-3 inside the root
  mha                  MultiHeadAttention(n_head, key_dim)(x, x): bias-added projections, the query scaled by 1 / sqrt(key_dim), value_dim =
                       key_dim, output projection back to d_model
  block_forward        modules.py:388-405 with every Dropout at rate 0
  stage_forward        modules.py:120-125
  variable_specs / forward / train_step   models.seldnet (models.py:18-32) with FIRST = mother_block | mother_stage (oracle.modules_oracle),
                       SECOND = transformer_encoder_block | _stage, heads / losses / Adam of oracle.seldnet_oracle (train.py:22-36)
"""
from __future__ import annotations

import copy
import math
from typing import Dict, List, Tuple

import numpy as np
import torch

from oracle import modules_oracle as M
from oracle import seldnet_oracle as O

LN_EPS = 1e-3
ACTS = {None: lambda t: t, "linear": lambda t: t, "relu": torch.relu, "tanh": torch.tanh, "sigmoid": torch.sigmoid,
        "swish": lambda t: t * torch.sigmoid(t)}


def attention(q, k, v, scale):
    """q, k, v [B, S, H, d] -> (o [B, S, H, d], lse [B, H, S])"""
    logits = torch.einsum("bnhd,bmhd->bhnm", q, k) * scale
    p = torch.softmax(logits, dim=-1)
    return torch.einsum("bhnm,bmhd->bnhd", p, v), torch.logsumexp(logits, dim=-1)


def layer_norm(x, gamma, beta, eps=LN_EPS):
    mean = x.mean(dim=-1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * gamma + beta


def block_specs(D: int, cfg: dict, prefix: str) -> List[Tuple[str, Tuple[int, ...]]]:
    """Keras creation order and shapes"""
    H, dk, k = int(cfg["n_head"]), int(cfg["key_dim"]), int(cfg["kernel_size"])
    F = int(cfg["ff_multiplier"] * D)
    out = []
    for part in ("query", "key", "value"):
        out += [(f"{prefix}.mha.{part}.kernel", (D, H, dk)), (f"{prefix}.mha.{part}.bias", (H, dk))]
    out += [(f"{prefix}.mha.attention_output.kernel", (H, dk, D)), (f"{prefix}.mha.attention_output.bias", (D,)),
            (f"{prefix}.ln0.gamma", (D,)), (f"{prefix}.ln0.beta", (D,)),
            (f"{prefix}.ffn0.kernel", (k, D, F)), (f"{prefix}.ffn0.bias", (F,)), (f"{prefix}.ffn1.kernel", (k, F, D)), (f"{prefix}.ffn1.bias", (D,)),
            (f"{prefix}.ln1.gamma", (D,)), (f"{prefix}.ln1.beta", (D,))]
    return out


def stage_specs(D: int, cfg: dict, depth: int, prefix: str = "tf"):
    return [s for i in range(depth) for s in block_specs(D, cfg, f"{prefix}{i}")]


def mha(x, w: Dict[str, torch.Tensor], prefix: str, cfg: dict):
    dk = int(cfg["key_dim"])
    proj = lambda part: torch.einsum("bsd,dhk->bshk", x, w[f"{prefix}.{part}.kernel"]) + w[f"{prefix}.{part}.bias"]
    o, _ = attention(proj("query"), proj("key"), proj("value"), 1.0 / math.sqrt(float(dk)))
    return torch.einsum("bshk,hkd->bsd", o, w[f"{prefix}.attention_output.kernel"]) + w[f"{prefix}.attention_output.bias"]


def block_forward(x, w: Dict[str, torch.Tensor], prefix: str, cfg: dict):
    """x [B, S, D]"""
    act = ACTS[cfg.get("activation", "relu")]
    x = layer_norm(x + mha(x, w, f"{prefix}.mha", cfg), w[f"{prefix}.ln0.gamma"], w[f"{prefix}.ln0.beta"])
    ffn = act(O.conv1d_same(x, w[f"{prefix}.ffn0.kernel"], w[f"{prefix}.ffn0.bias"]))
    ffn = O.conv1d_same(ffn, w[f"{prefix}.ffn1.kernel"], w[f"{prefix}.ffn1.bias"])
    return layer_norm(x + ffn, w[f"{prefix}.ln1.gamma"], w[f"{prefix}.ln1.beta"])


def stage_forward(x, w, cfg: dict, depth: int, prefix: str = "tf"):
    for i in range(depth):
        x = block_forward(x, w, f"{prefix}{i}", cfg)
    return x


def random_block_weights(specs, seed: int) -> np.ndarray:
    """glorot-uniform kernels; biases, gamma and beta perturbed so that they matter"""
    rng = np.random.default_rng(seed)
    out = []
    for name, sh in specs:
        n = int(np.prod(sh))
        if name.endswith("kernel"):
            fan_in = int(np.prod(sh[:-1]))
            fan_out = int(sh[-1]) * (int(np.prod(sh[:-2])) if len(sh) > 2 else 1)
            out.append(rng.uniform(-1, 1, n) * math.sqrt(6.0 / (fan_in + fan_out)))
        elif name.endswith("gamma"):
            out.append(1.0 + 0.1 * rng.standard_normal(n))
        else:
            out.append(0.05 * rng.standard_normal(n))
    return np.concatenate(out).astype(np.float32)


# ---- models.seldnet with a mother FIRST block and a transformer SECOND block
def _depth(model_config: dict) -> int:
    if model_config["SECOND"] == "transformer_encoder_stage":
        return int(model_config["SECOND_ARGS"]["depth"])
    if model_config["SECOND"] == "transformer_encoder_block":
        return 1
    raise ValueError("transformer_oracle restates transformer_encoder_block / transformer_encoder_stage as SECOND")


def _gru_less(model_config: dict) -> dict:
    """the same configuration with an EMPTY recurrent stage: oracle.modules_oracle then restates FIRST and the heads around ours"""
    mc = copy.deepcopy(model_config)
    mc["SECOND"], mc["SECOND_ARGS"] = "bidirectional_GRU_block", {"units": []}
    return mc


def variable_specs(model_config: dict, input_shape):
    tr, nt = M.variable_specs(_gru_less(model_config), input_shape)
    shape = tuple(int(v) for v in input_shape[-3:])
    for d, cfg in enumerate(M.first_configs(model_config)):
        _, _, shape = M.mother_block_plan(cfg, shape, f"mb{d}")
    n_first = next(i for i, (n, _) in enumerate(tr + [("sed.", ())]) if n.startswith(("sed.", "doa.")))
    mid = stage_specs(shape[1] * shape[2], model_config["SECOND_ARGS"], _depth(model_config))
    return tr[:n_first] + mid + tr[n_first:], nt


def random_weights(model_config: dict, input_shape, seed: int = 0):
    tr, nt = variable_specs(model_config, input_shape)
    w0, st = M.random_weights(_gru_less(model_config), input_shape, seed)
    tr0, _ = M.variable_specs(_gru_less(model_config), input_shape)
    d0 = {n: w0[o:o + int(np.prod(s))] for (n, s), o in zip(tr0, np.cumsum([0] + [int(np.prod(s)) for _, s in tr0])[:-1])}
    mid = [(n, s) for n, s in tr if n.startswith("tf")]
    wm = random_block_weights(mid, seed + 1)
    dm = {n: wm[o:o + int(np.prod(s))] for (n, s), o in zip(mid, np.cumsum([0] + [int(np.prod(s)) for _, s in mid])[:-1])}
    return np.concatenate([dm[n] if n in dm else d0[n] for n, _ in tr]).astype(np.float32), st


def forward(model_config: dict, w, st, x, training: bool):
    """-> (sed, doa, new_state)"""
    new_st = dict(st)
    h = x
    for d, cfg in enumerate(M.first_configs(model_config)):
        h = M.mother_block_forward(cfg, w, st, new_st, h, training, f"mb{d}")
    B, S = h.shape[0], h.shape[1]
    h = h.reshape(B, S, -1)          # layers.force_1d_inputs (layers.py:41-47)
    h = stage_forward(h, w, model_config["SECOND_ARGS"], _depth(model_config))
    sp = M._tail_spec(_gru_less(model_config))
    outs = []
    for head, units, act, hact in (("sed", sp.sed_units, torch.sigmoid, ACTS[sp.sed_dense_act]), ("doa", sp.doa_units, torch.tanh, ACTS[sp.doa_dense_act])):
        a = h
        for j in range(len(units)):
            a = hact(a @ w[f"{head}.dense{j}.kernel"][0] + w[f"{head}.dense{j}.bias"])
        outs.append(act(a @ w[f"{head}.out.kernel"] + w[f"{head}.out.bias"]))
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
    ns = torch.cat([new_st[n].detach().reshape(-1) for n, _ in nt]) if nt else torch.zeros(0, dtype=dtype)
    return {"sed": sed.detach().numpy(), "doa": doa.detach().numpy(), "sloss": sloss.detach().numpy(), "dloss": dloss.detach().numpy(),
            "grad": g.numpy(), "new_w": new_w.numpy(), "new_state": ns.numpy()}


# ---- deterministic stress inputs for the attention and LayerNorm operators (tests/test_attention_cpu.py holds the condition a plain fp32
# evaluation meets on each of them, tests/test_attention_gpu.py runs the device on the same arrays)
def f32(a) -> np.ndarray:
    """the fp32-rounded values as float64: what the device receives, so that input rounding is not charged to the kernel"""
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


# (kind, span, B, S, H, d): S of three tiles or more, one narrow and one wide head
STRESS_CASES = [("gain", 0, 2, 130, 3, 16), ("gain", 0, 2, 130, 2, 64)] + [
    (kind, span, 2, 200, 2, d) for d in (16, 64) for kind, span in (("ramp_up", 60), ("ramp_down", 60), ("ramp_up", 100), ("ramp_down", 100),
                                                                    ("shifted", 60))]


def stress_qkv(kind: str, span: float, B: int, S: int, H: int, d: int):
    """-> (q, k, v, do [B, S, H, d] float64 holding fp32 values, scale = 1 / sqrt(d)).
      gain       q and k unit-normal times 3: logits of tens, most rows one dominant key
      ramp_up    component 0 of every query is 2 and component 0 of key j adds span * j / (S - 1) to its logit: the running maximum rises
                 from key block to key block
      ramp_down  ... adds span * (1 - j / (S - 1)): the late tiles underflow against the first
      shifted    ramp_down with every key's component 0 lowered until every logit of every row is below -90: a softmax without the
                 maximum subtraction sums zeros"""
    rng = np.random.default_rng([S, H, d, int(span), len(kind)])
    q, k, v, do = (rng.standard_normal((B, S, H, d)) for _ in range(4))
    scale = 1.0 / math.sqrt(d)
    if kind == "gain":
        q, k = 3.0 * q, 3.0 * k
    elif kind in ("ramp_up", "ramp_down", "shifted"):
        j = np.arange(S, dtype=np.float64) / max(S - 1, 1)
        ramp = span * (j if kind == "ramp_up" else 1.0 - j)
        q[..., 0] = 2.0
        k[..., 0] = (ramp / (2.0 * scale))[None, :, None]
        if kind == "shifted":
            top = float((np.einsum("bnhd,bmhd->bhnm", f32(q), f32(k)) * scale).max())
            k[..., 0] -= (math.ceil(top) + 95.0) / (2.0 * scale)
    else:
        raise ValueError(kind)
    return f32(q), f32(k), f32(v), f32(do), scale


# (mean, std, rows, C)
LN_OFFSET_CASES = [(10.0, 0.1, 40, 128), (10.0, 0.1, 40, 257), (100.0, 1.0, 40, 128), (100.0, 1.0, 12, 4378)]


def offset_rows(mean: float, std: float, rows: int, C: int):
    """-> (x, r, dy [rows, C], gamma, beta [C]) float64 holding fp32 values.  x + r has the given mean and standard deviation per row —
    where a one-pass E[z^2] - mean^2 in fp32 loses the variance — gamma spans three decades and beta sits at 50.  Row 1 of x + r is exactly
    constant although neither x nor r is (r = mean - x there, in fp32 values whose sum is exact), and row 2 of x is constant with r = 0."""
    rng = np.random.default_rng([rows, C, int(mean)])
    z = mean + std * rng.standard_normal((rows, C))
    r = 0.25 * mean + 0.5 * std * rng.standard_normal((rows, C))
    x = f32(z - f32(r))
    r = f32(r)
    if rows > 2:
        x[1] = np.round(rng.uniform(1, 3, C) * 64) / 64          # multiples of 1 / 64: x + r = mean exactly, in fp32 as well
        r[1] = mean - x[1]
        x[2], r[2] = mean, 0.0
    dy = rng.standard_normal((rows, C))
    gamma = 10.0 ** rng.uniform(-1.5, 1.5, C) * np.where(rng.random(C) < 0.5, -1.0, 1.0)
    beta = 50.0 + rng.standard_normal(C)
    return x, r, f32(dy), f32(gamma), f32(beta)
