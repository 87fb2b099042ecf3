"""fp64 restatement (torch, CPU) of what seld_amd/modules.py adds for the reference's conformer_encoder_block / _stage (modules.py:129-152,
410-508) with every Dropout at rate 0.  A helper, not a test file: tests/test_conformer_cpu.py pins it against torch's own operators, and
tests/test_conformer_gpu.py checks the device against it.

  glu                    tf.split(conv, 2, -1); conv_1 * sigmoid(conv_2) (modules.py:476-478); the sigmoid in a form whose autograd derivative
                         keeps its value where the gate saturates
  depthwise_conv1d       Conv1D(filters = C, kernel_size k, 'same', groups = C) (modules.py:481-486): Keras' kernel [k, 1, C]; TensorFlow's 'same'
                         pads (k - 1) // 2 frames in front and the rest behind
  pos_table              layers.basic_pos_encoding (layers.py:53-67): w_i = float32(10000 ** (-i / (D // 2))), cos / sin interleaved per
                         frequency; w t, cos and sin in float64, rounded to float32 once (the model constant both sides use)
  mha_ref                layers.MultiHeadAttention_ (layers.py:102-287): head-major kernels [H, D, dk], the query divided by sqrt(dk) after its bias
  block_forward          modules.py:432-506; the last residual adds to x, not to x + conv (modules.py:495, 504)
  variable_specs / random_weights / forward / train_step   models.seldnet (models.py:18-32) with FIRST = mother_block | mother_stage
                         (oracle.modules_oracle), SECOND = conformer_encoder_block | _stage, heads / losses / Adam of oracle.seldnet_oracle
"""
from __future__ import annotations

import copy
import math
from typing import Dict

import numpy as np
import torch

import transformer_oracle as T
from oracle import modules_oracle as M
from oracle import seldnet_oracle as O

ACTS = T.ACTS
f32 = T.f32


def sigmoid(b):
    """torch.sigmoid's values from e = exp(-|b|) <= 1, so that autograd's derivative is e / (1 + e)^2 and not s (1 - s) on a rounded s: at
    b = 40 the latter is 0 in float64 as well (1 - 4.2e-18 rounds to 1), where the derivative is 4.2e-18"""
    pos = b >= 0
    e = torch.exp(torch.where(pos, -b, b))      # not -|b|: autograd gives |b| the slope 0 at b = 0
    r = 1.0 / (1.0 + e)
    return torch.where(pos, r, e * r)


def glu(u):
    a, b = torch.split(u, u.shape[-1] // 2, dim=-1)
    return a * sigmoid(b)


def depthwise_conv1d(g, kernel, bias):
    """g [B, S, C], kernel [k, 1, C] (or [k, C]), bias [C]"""
    k, S = kernel.shape[0], g.shape[1]
    kernel = kernel.reshape(k, -1)
    pl = (k - 1) // 2
    gp = torch.nn.functional.pad(g, (0, 0, pl, k - 1 - pl))
    return sum(gp[:, t:t + S] * kernel[t] for t in range(k)) + bias


def pos_table(S: int, D: int) -> np.ndarray:
    """[S, 2 (D // 2)] float32"""
    k = D // 2
    w = np.float32(10000.0) ** (-np.arange(k, dtype=np.float64) / k)
    w = w.astype(np.float32).astype(np.float64)
    arg = np.arange(S, dtype=np.float64)[:, None] * w[None, :]
    out = np.empty((S, k, 2), np.float64)
    out[:, :, 0], out[:, :, 1] = np.cos(arg), np.sin(arg)
    return out.reshape(S, 2 * k).astype(np.float32)


def cfg_get(cfg: dict):
    """the defaults of modules.py:412-421"""
    return {"key_dim": int(cfg.get("key_dim", 36)), "n_head": int(cfg.get("n_head", 4)), "kernel_size": int(cfg.get("kernel_size", 32)),
            "activation": cfg.get("activation", "swish"), "multiplier": int(cfg.get("multiplier", 4)), "ffn_factor": float(cfg.get("ffn_factor", 0.5)),
            "pos_encoding": cfg.get("pos_encoding", "basic"), "use_bias": bool(cfg.get("use_bias", True))}


def block_specs(D: int, cfg: dict, prefix: str):
    """-> (trainable, state) [(name, shape)] in Keras creation order"""
    c = cfg_get(cfg)
    H, dk, k, F = c["n_head"], c["key_dim"], c["kernel_size"], c["multiplier"] * D
    ln = lambda n: [(f"{prefix}.{n}.gamma", (D,)), (f"{prefix}.{n}.beta", (D,))]
    ffn = lambda n: [(f"{prefix}.{n}a.kernel", (D, F)), (f"{prefix}.{n}a.bias", (F,)), (f"{prefix}.{n}b.kernel", (F, D)), (f"{prefix}.{n}b.bias", (D,))]
    mha = [(f"{prefix}.mha.{p}_kernel", (H, D, dk)) for p in ("query", "key", "value")] + [(f"{prefix}.mha.projection_kernel", (H, dk, D))]
    if c["use_bias"]:
        mha += [(f"{prefix}.mha.projection_bias", (D,))] + [(f"{prefix}.mha.{p}_bias", (H, dk)) for p in "qkv"]
    tr = (ln("ln0") + ffn("ffn0") + ln("ln1") + mha + ln("ln2") + [(f"{prefix}.pw0.kernel", (1, D, 2 * D)), (f"{prefix}.pw0.bias", (2 * D,)),
          (f"{prefix}.dw.kernel", (k, 1, D)), (f"{prefix}.dw.bias", (D,)), (f"{prefix}.bn.gamma", (D,)), (f"{prefix}.bn.beta", (D,)),
          (f"{prefix}.pw1.kernel", (1, D, D)), (f"{prefix}.pw1.bias", (D,))] + ln("ln3") + ffn("ffn1") + ln("ln4"))
    nt = [(f"{prefix}.bn.moving_mean", (D,)), (f"{prefix}.bn.moving_variance", (D,))]
    return tr, nt


def stage_specs(D: int, cfg: dict, depth: int, prefix: str = "cf"):
    tr, nt = [], []
    for i in range(depth):
        t, n = block_specs(D, cfg, f"{prefix}{i}")
        tr += t
        nt += n
    return tr, nt


def mha_ref(x, w: Dict[str, torch.Tensor], prefix: str, cfg: dict):
    c = cfg_get(cfg)
    q, k, v = (torch.einsum("bnd,hdo->bnho", x, w[f"{prefix}.{p}_kernel"]) for p in ("query", "key", "value"))
    if c["use_bias"]:
        q, k, v = q + w[f"{prefix}.q_bias"], k + w[f"{prefix}.k_bias"], v + w[f"{prefix}.v_bias"]
    q = q / math.sqrt(float(c["key_dim"]))
    o, _ = T.attention(q, k, v, 1.0)
    out = torch.einsum("bnhi,hio->bno", o, w[f"{prefix}.projection_kernel"])
    return out + w[f"{prefix}.projection_bias"] if c["use_bias"] else out


def block_forward(x, w, st, new_st, prefix: str, cfg: dict, training: bool):
    """x [B, S, D]; st / new_st: the BatchNormalization statistics read / written"""
    c = cfg_get(cfg)
    act, ff = ACTS[c["activation"]], c["ffn_factor"]
    ln = lambda n, t: T.layer_norm(t, w[f"{prefix}.{n}.gamma"], w[f"{prefix}.{n}.beta"])
    dense = lambda n, t: t @ w[f"{prefix}.{n}.kernel"].reshape(-1, w[f"{prefix}.{n}.kernel"].shape[-1]) + w[f"{prefix}.{n}.bias"]
    ffn = lambda n, t: dense(n + "b", act(dense(n + "a", t)))
    x = x + ff * ffn("ffn0", ln("ln0", x))
    if c["pos_encoding"] == "basic":
        x = x + torch.as_tensor(pos_table(x.shape[1], x.shape[2])).to(x.dtype)
    x = x + mha_ref(ln("ln1", x), w, f"{prefix}.mha", cfg)
    conv = depthwise_conv1d(glu(dense("pw0", ln("ln2", x))), w[f"{prefix}.dw.kernel"], w[f"{prefix}.dw.bias"])
    y, m, v = O.batchnorm(conv[:, :, None, :], w[f"{prefix}.bn.gamma"], w[f"{prefix}.bn.beta"], st[f"{prefix}.bn.moving_mean"],
                          st[f"{prefix}.bn.moving_variance"], training)
    new_st[f"{prefix}.bn.moving_mean"], new_st[f"{prefix}.bn.moving_variance"] = m, v
    conv = dense("pw1", ACTS["swish"](y[:, :, 0, :])) + x
    return ln("ln4", x + ff * ffn("ffn1", ln("ln3", conv)))


def stage_forward(x, w, st, new_st, cfg: dict, depth: int, training: bool, prefix: str = "cf"):
    for i in range(depth):
        x = block_forward(x, w, st, new_st, f"{prefix}{i}", cfg, training)
    return x


def random_stage_weights(D: int, cfg: dict, depth: int, seed: int, prefix: str = "cf"):
    """-> (flat trainable, flat state) float32: T.random_block_weights' rules; moving statistics away from 0 / 1"""
    tr, nt = stage_specs(D, cfg, depth, prefix)
    rng = np.random.default_rng(seed + 7)
    st = [0.1 * rng.standard_normal(int(np.prod(s))) if n.endswith("moving_mean") else 1.0 + 0.3 * rng.random(int(np.prod(s))) for n, s in nt]
    return T.random_block_weights(tr, seed), np.concatenate(st).astype(np.float32)


# ---- models.seldnet with a mother FIRST block and a conformer SECOND block
def _depth(model_config: dict) -> int:
    if model_config["SECOND"] == "conformer_encoder_stage":
        return int(model_config["SECOND_ARGS"]["depth"])
    if model_config["SECOND"] == "conformer_encoder_block":
        return 1
    raise ValueError("conformer_oracle restates conformer_encoder_block / conformer_encoder_stage as SECOND")


def _first_out(model_config: dict, input_shape):
    shape = tuple(int(v) for v in input_shape[-3:])
    for d, cfg in enumerate(M.first_configs(model_config)):
        _, _, shape = M.mother_block_plan(cfg, shape, f"mb{d}")
    return shape


def variable_specs(model_config: dict, input_shape):
    gl = T._gru_less(model_config)
    tr, nt = M.variable_specs(gl, input_shape)
    shape = _first_out(model_config, input_shape)
    n_first = next(i for i, (n, _) in enumerate(tr + [("sed.", ())]) if n.startswith(("sed.", "doa.")))
    mid, mid_nt = stage_specs(shape[1] * shape[2], model_config["SECOND_ARGS"], _depth(model_config))
    return tr[:n_first] + mid + tr[n_first:], nt + mid_nt


def random_weights(model_config: dict, input_shape, seed: int = 0):
    gl = T._gru_less(model_config)
    tr, nt = variable_specs(model_config, input_shape)
    w0, st0 = M.random_weights(gl, input_shape, seed)
    tr0, _ = M.variable_specs(gl, input_shape)
    flat = lambda specs, a: {n: a[o:o + int(np.prod(s))] for (n, s), o in zip(specs, np.cumsum([0] + [int(np.prod(s)) for _, s in specs])[:-1])}
    d0 = flat(tr0, w0)
    shape = _first_out(model_config, input_shape)
    D, depth = shape[1] * shape[2], _depth(model_config)
    mid, _ = stage_specs(D, model_config["SECOND_ARGS"], depth)
    wm, sm = random_stage_weights(D, model_config["SECOND_ARGS"], depth, seed + 1)
    dm = flat(mid, wm)
    return np.concatenate([dm[n] if n in dm else d0[n] for n, _ in tr]).astype(np.float32), np.concatenate([st0, sm]).astype(np.float32)


def forward(model_config: dict, w, st, x, training: bool):
    """-> (sed, doa, new_state)"""
    new_st = dict(st)
    h = x
    for d, cfg in enumerate(M.first_configs(model_config)):
        h = M.mother_block_forward(cfg, w, st, new_st, h, training, f"mb{d}")
    B, S = h.shape[0], h.shape[1]
    h = h.reshape(B, S, -1)          # layers.force_1d_inputs (layers.py:41-47)
    h = stage_forward(h, w, st, new_st, model_config["SECOND_ARGS"], _depth(model_config), training)
    sp = M._tail_spec(T._gru_less(model_config))
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
    ns = torch.cat([new_st[n].detach().reshape(-1) for n, _ in nt])
    return {"sed": sed.detach().numpy(), "doa": doa.detach().numpy(), "sloss": sloss.detach().numpy(), "dloss": dloss.detach().numpy(),
            "grad": g.numpy(), "new_w": new_w.numpy(), "new_state": ns.numpy()}


# ---- the block / stage cases of tests/test_conformer_gpu.py (tests/test_conformer_cpu.py holds that a plain fp32 evaluation of each stays within
# 5e-5 of fp64): (B, S, D, depth, cfg)
def _cfg(H, dk, k, m, **kw):
    return dict({"n_head": H, "key_dim": dk, "kernel_size": k, "multiplier": m, "dropout_rate": 0}, **kw)


STAGE_CASES = {
    "reference shape": (2, 600, 128, 1, _cfg(4, 32, 32, 4, pos_encoding="basic")),
    "SS5 first": (2, 100, 96, 2, _cfg(4, 24, 24, 2, depth=2, pos_encoding=None)),
    "SS5 second": (2, 100, 96, 1, _cfg(4, 48, 8, 2, depth=1, pos_encoding=None)),
    "odd sizes": (3, 61, 72, 1, _cfg(4, 40, 7, 4)),
    "no biases": (2, 33, 50, 1, _cfg(5, 8, 8, 4, use_bias=False)),
    "one frame": (2, 1, 48, 1, _cfg(4, 16, 32, 4)),
    "ffn_factor 1 relu": (2, 40, 64, 1, _cfg(4, 16, 5, 2, ffn_factor=1.0, activation="relu")),
    "ffn_factor 0.5 swish": (2, 40, 64, 1, _cfg(4, 16, 5, 2, ffn_factor=0.5, activation="swish")),
}


def stage_reference(B, S, D, depth, cfg, seed, dtype=torch.float64):
    """-> dict: x, dy, w, st (numpy inputs), out_train, out_eval (inference on the statistics the training step left), new_state, dx, grad"""
    tr, nt = stage_specs(D, cfg, depth)
    w, st = random_stage_weights(D, cfg, depth, seed)
    rng = np.random.default_rng(seed)
    x, dy = f32(rng.standard_normal((B, S, D))), f32(rng.standard_normal((B, S, D)))
    fw = torch.tensor(w, dtype=dtype, requires_grad=True)
    xt = torch.tensor(x, dtype=dtype, requires_grad=True)
    sd = O.unflatten(torch.tensor(st, dtype=dtype), nt)
    new_st = dict(sd)
    yt = stage_forward(xt, O.unflatten(fw, tr), sd, new_st, cfg, depth, True)
    gw, gx = torch.autograd.grad((yt * torch.tensor(dy, dtype=dtype)).sum(), (fw, xt))
    with torch.no_grad():
        ye = stage_forward(xt, O.unflatten(fw, tr), new_st, dict(new_st), cfg, depth, False)
    ns = torch.cat([new_st[n].detach().reshape(-1) for n, _ in nt])
    return {"x": x, "dy": dy, "w": w, "st": st, "out_train": yt.detach().numpy(), "out_eval": ye.numpy(), "new_state": ns.numpy(),
            "dx": gx.numpy(), "grad": gw.numpy(), "specs": (tr, nt)}


# ---- deterministic inputs for the depthwise kernels
def dwconv_inputs(B, S, C, k, glu: bool, seed: int, gate_span: float = 0.0):
    """-> (u [B, S, (1 + glu) C], w [k, C], bias [C], dy [B, S, C]) float64 holding fp32 values.  gate_span > 0: the gate half of u is spread
    over [-gate_span, gate_span] (sigmoid saturated on both sides: a derivative formed as s (1 - s) from a rounded s, or an exp that
    overflows, shows), with every 7th gate at exactly +-gate_span"""
    rng = np.random.default_rng([B, S, C, k, int(glu), seed])
    u = rng.standard_normal((B, S, (1 + int(glu)) * C))
    if glu and gate_span > 0:
        gate = rng.uniform(-gate_span, gate_span, (B, S, C))
        flat = gate.reshape(-1)
        flat[::7] = np.where(np.arange(flat[::7].size) % 2 == 0, gate_span, -gate_span)
        u[..., C:] = gate
    w = rng.standard_normal((k, C)) / math.sqrt(k)
    return f32(u), f32(w), f32(0.3 * rng.standard_normal(C)), f32(rng.standard_normal((B, S, C)))


def dwconv_reference(u, w, bias, dy, glu: bool, dtype=torch.float64):
    """-> (y, du, dw, dbias) numpy"""
    tu, tw, tb = (torch.tensor(a, dtype=dtype, requires_grad=True) for a in (u, w, bias))
    y = depthwise_conv1d(globals()["glu"](tu) if glu else tu, tw, tb)
    gu, gw, gb = torch.autograd.grad((y * torch.tensor(dy, dtype=dtype)).sum(), (tu, tw, tb))
    return y.detach().numpy(), gu.numpy(), gw.numpy(), gb.numpy()
