"""fp64 restatement (torch, CPU) of what seld_amd/modules.py adds for the reference's attention_block / attention_stage (modules.py:155-180,
511-635) and layers.RelPositionMultiHeadAttention (layers.py:332-392), every Dropout at rate 0.  A helper, not a test file:
tests/test_attention_block_cpu.py pins it, tests/test_attention_block_gpu.py checks the device against it.

  relative_shift         the literal form of layers.py:360-365: pad one zero column in front, reshape [.., N, M + 1] -> [.., M + 1, N], drop the
                         first row, reshape back
  shift_closed_form      the index identity seld_amd/csrc/relattn.hip runs on: shifted[i,j] = G[i, S-1-i+j] (j <= i), 0 (j = i+1),
                         G[i+1, j-i-2] (j >= i+2)
  use_once_map           where each G[i,m] is read (the backward of the shift as a re-indexing)
  rel_attention          the core on projected q, k, v [B,S,H,d], P [S,H,d], u, vb [H,d] -> (O, lse): what seld_relattn_fwd computes
  rel_mha                the layer: head-major kernels, pos_kernel / pos_bias_u / pos_bias_v first (layers.py:333-357)
  block_specs / block_forward / stage_*   modules.attention_block with the reference's quirks
  variable_specs / random_weights / forward / train_step   models.seldnet with a mother FIRST block and SECOND = attention_block | _stage
"""
from __future__ import annotations

import math
from typing import Dict

import numpy as np
import torch

import conformer_oracle as CF
import transformer_oracle as T
from oracle import modules_oracle as M
from oracle import seldnet_oracle as O

ACTS = T.ACTS
f32 = T.f32


# ---------------------------------------------------------------- the shift
def relative_shift(x):
    """x [B, H, N, M] -> [B, H, N, M] (layers.py:360-365)"""
    b, h, n, m = x.shape
    x = torch.nn.functional.pad(x, (1, 0))
    x = x.reshape(b, h, m + 1, n)
    return x[:, :, 1:, :].reshape(b, h, n, m)


def shift_closed_form(G):
    """G [.., S, S] -> shifted [.., S, S] by the index identity (N = M = S)"""
    S = G.shape[-1]
    out = torch.zeros_like(G)
    for i in range(S):
        for j in range(S):
            if j <= i:
                out[..., i, j] = G[..., i, S - 1 - i + j]
            elif j >= i + 2:
                out[..., i, j] = G[..., i + 1, j - i - 2]
    return out


def use_once_map(S: int):
    """-> {(i, m): (i', j)}: the one logit (i', j) that reads G[i, m]; G[0, m <= S - 2] is read by none"""
    out = {}
    for i in range(S):
        for m in range(S):
            if m >= S - 1 - i:
                out[(i, m)] = (i, m - S + 1 + i)
            elif i >= 1:
                out[(i, m)] = (i - 1, m + i + 1)
    return out


def rel_attention(q, k, v, P, u, vb, scale):
    """q, k, v [B,S,H,d]; P [S,H,d]; u, vb [H,d] -> (O [B,S,H,d], lse [B,H,S])"""
    a = torch.einsum("bnho,bmho->bhnm", q + u, k)
    g = torch.einsum("bnho,mho->bhnm", q + vb, P)
    logits = (a + relative_shift(g)[:, :, :, :a.shape[3]]) * scale
    p = torch.softmax(logits, dim=-1)
    return torch.einsum("bhnm,bmhd->bnhd", p, v), torch.logsumexp(logits, dim=-1)


def relattn_inputs(B, S, H, d, seed=0):
    """-> q, k, v [B,S,H,d], P [S,H,d], u, vb [H,d], dO [B,S,H,d] float64 holding fp32 values, scale.  Logits of a few units: a softmax that is
    neither flat nor one-hot."""
    rng = np.random.default_rng([B, S, H, d, seed])
    g = lambda *s: f32(rng.standard_normal(s))
    q, k, v, do = g(B, S, H, d), g(B, S, H, d), g(B, S, H, d), g(B, S, H, d)
    return q, k, v, g(S, H, d), 0.5 * g(H, d), 0.5 * g(H, d), do, 1.0 / math.sqrt(d)


def relattn_reference(q, k, v, P, u, vb, do, scale, dtype=torch.float64):
    """-> dict of numpy: O, lse, dQu, dQv, dK, dV, dP (dQu / dQv: the gradients of q + u and q + vb)"""
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    tq, tk, tv, tp = (t(a).requires_grad_(True) for a in (q, k, v, P))
    qu = (tq + t(u)).detach().requires_grad_(True)
    qv = (tq + t(vb)).detach().requires_grad_(True)
    a = torch.einsum("bnho,bmho->bhnm", qu, tk)
    g = torch.einsum("bnho,mho->bhnm", qv, tp)
    logits = (a + relative_shift(g)) * scale
    o = torch.einsum("bhnm,bmhd->bnhd", torch.softmax(logits, dim=-1), tv)
    gs = torch.autograd.grad((o * t(do)).sum(), (qu, qv, tk, tv, tp))
    out = {"O": o, "lse": torch.logsumexp(logits, dim=-1)}
    out.update(zip(("dQu", "dQv", "dK", "dV", "dP"), gs))
    return {n: a.detach().numpy() for n, a in out.items()}


# ---------------------------------------------------------------- the layer and the block
def cfg_get(cfg: dict):
    """the mandatory keys and the defaults of modules.py:513-529"""
    return {"key_dim": int(cfg["key_dim"]), "n_head": int(cfg["n_head"]), "kernel_size": int(cfg["kernel_size"]),
            "ff_kernel_size": int(cfg["ff_kernel_size"]), "ff_multiplier": cfg["ff_multiplier"], "ff_factor0": float(cfg["ff_factor0"]),
            "ff_factor1": float(cfg["ff_factor1"]), "activation": cfg.get("activation", "swish"), "pos_encoding": cfg.get("pos_encoding", "basic"),
            "abs_pos_encoding": bool(cfg.get("abs_pos_encoding", False)), "layer_norm_in_front": bool(cfg.get("layer_norm_in_front", False)),
            "use_glu": bool(cfg.get("use_glu", False)), "use_bias": bool(cfg.get("use_bias", False))}


def mha_specs(D, c, prefix):
    H, dk = c["n_head"], c["key_dim"]
    out = []
    if not c["abs_pos_encoding"]:
        out += [(f"{prefix}.pos_kernel", (H, D, dk)), (f"{prefix}.pos_bias_u", (H, dk)), (f"{prefix}.pos_bias_v", (H, dk))]
    out += [(f"{prefix}.{p}_kernel", (H, D, dk)) for p in ("query", "key", "value")] + [(f"{prefix}.projection_kernel", (H, dk, D))]
    if c["use_bias"]:
        out += [(f"{prefix}.projection_bias", (D,))] + [(f"{prefix}.{p}_bias", (H, dk)) for p in "qkv"]
    return out


def block_specs(D: int, cfg: dict, prefix: str):
    """-> (trainable, state) [(name, shape)] in the creation order of the LIVE layers (the LayerNormalization in front of a FF module is dead:
    its output is discarded, modules.py:561-565, 621-625)"""
    c = cfg_get(cfg)
    k, fk, F, lnf = c["kernel_size"], c["ff_kernel_size"], int(c["ff_multiplier"] * D), c["layer_norm_in_front"]
    ln = lambda n: [(f"{prefix}.{n}.gamma", (D,)), (f"{prefix}.{n}.beta", (D,))]
    conv = lambda n, ks, a, b: [(f"{prefix}.{n}.kernel", (ks, a, b)), (f"{prefix}.{n}.bias", (b,))]
    ff = lambda n, lname: conv(n + "a", fk, D, F) + conv(n + "b", fk, F, D) + ([] if lnf else ln(lname))
    tr, nt = [], []
    if c["ff_factor0"] > 0:
        tr += ff("ff0", "ln0")
    tr += (ln("ln1") if lnf else []) + mha_specs(D, c, f"{prefix}.mha") + ([] if lnf else ln("ln1"))
    if c["use_glu"]:
        tr += (ln("ln2") if lnf else []) + conv("pw0", 1, D, 2 * D)
    if k > 0:
        tr += (ln("ln2") if lnf and not c["use_glu"] else []) + conv("dw", k, 1, D) + [(f"{prefix}.bn.gamma", (D,)), (f"{prefix}.bn.beta", (D,))]
        tr += conv("pw1", 1, D, D) + ([] if lnf else ln("ln2"))
        nt += [(f"{prefix}.bn.moving_mean", (D,)), (f"{prefix}.bn.moving_variance", (D,))]
    if c["ff_factor1"] > 0:
        tr += ff("ff1", "ln3")
    return tr, nt


def stage_specs(D: int, cfg: dict, depth: int, prefix: str = "at"):
    tr, nt = [], []
    for i in range(depth):
        t, n = block_specs(D, cfg, f"{prefix}{i}")
        tr += t
        nt += n
    return tr, nt


def conv1d_same(x, kernel, bias):
    """Conv1D(filters, k, padding='same') on [B, S, Cin]; kernel [k, Cin, N]"""
    k, S = kernel.shape[0], x.shape[1]
    pl = (k - 1) // 2
    xp = torch.nn.functional.pad(x, (0, 0, pl, k - 1 - pl))
    return sum(xp[:, t:t + S] @ kernel[t] for t in range(k)) + bias


def rel_mha(x, pos, w: Dict[str, torch.Tensor], prefix: str, c: dict):
    """layers.RelPositionMultiHeadAttention([x, x, x, pos]) (layers.py:367-392); pos [S, D]"""
    q, k, v = (torch.einsum("bnd,hdo->bnho", x, w[f"{prefix}.{p}_kernel"]) for p in ("query", "key", "value"))
    if c["use_bias"]:
        q, k, v = q + w[f"{prefix}.q_bias"], k + w[f"{prefix}.k_bias"], v + w[f"{prefix}.v_bias"]
    P = torch.einsum("md,hdo->mho", pos, w[f"{prefix}.pos_kernel"])
    o, _ = rel_attention(q, k, v, P, w[f"{prefix}.pos_bias_u"], w[f"{prefix}.pos_bias_v"], 1.0 / math.sqrt(float(c["key_dim"])))
    out = torch.einsum("bnhi,hio->bno", o, w[f"{prefix}.projection_kernel"])
    return out + w[f"{prefix}.projection_bias"] if c["use_bias"] else out


def block_forward(x, w, st, new_st, prefix: str, cfg: dict, training: bool):
    """modules.py:553-634 on x [B, S, D]"""
    c = cfg_get(cfg)
    act, lnf, k = ACTS[c["activation"]], c["layer_norm_in_front"], c["kernel_size"]
    ln = lambda n, t: T.layer_norm(t, w[f"{prefix}.{n}.gamma"], w[f"{prefix}.{n}.beta"])
    conv = lambda n, t: conv1d_same(t, w[f"{prefix}.{n}.kernel"], w[f"{prefix}.{n}.bias"])
    ff = lambda n, t: conv(n + "b", act(conv(n + "a", t)))          # reads x, not the LayerNormalization in front (quirk 1)
    if c["ff_factor0"] > 0:
        x = x + c["ff_factor0"] * ff("ff0", x)
        if not lnf:
            x = ln("ln0", x)
    attn = x                                                           # taken before the table is added (quirk 2)
    pos = torch.as_tensor(CF.pos_table(x.shape[1], x.shape[2])).to(x.dtype) if c["pos_encoding"] == "basic" else None
    if lnf:
        attn = ln("ln1", attn)
    if c["abs_pos_encoding"]:
        if pos is not None:
            x = x + pos
        attn = CF.mha_ref(attn, w, f"{prefix}.mha", {"key_dim": c["key_dim"], "n_head": c["n_head"], "use_bias": c["use_bias"]})
    else:
        attn = rel_mha(attn, pos, w, f"{prefix}.mha", c)
    x = attn + x
    if not lnf:
        x = ln("ln1", x)
    cv = x
    if c["use_glu"]:
        if lnf:
            cv = ln("ln2", cv)
        cv = CF.glu(conv("pw0", cv))
    if k > 0:
        if lnf and not c["use_glu"]:
            cv = ln("ln2", cv)
        cv = CF.depthwise_conv1d(cv, w[f"{prefix}.dw.kernel"], w[f"{prefix}.dw.bias"])
        y, m, v = O.batchnorm(cv[:, :, None, :], w[f"{prefix}.bn.gamma"], w[f"{prefix}.bn.beta"], st[f"{prefix}.bn.moving_mean"],
                              st[f"{prefix}.bn.moving_variance"], training)
        new_st[f"{prefix}.bn.moving_mean"], new_st[f"{prefix}.bn.moving_variance"] = m, v
        x = x + conv("pw1", ACTS["swish"](y[:, :, 0, :]))
        if not lnf:
            x = ln("ln2", x)
    else:
        x = cv                                                         # no residual, no LayerNormalization (quirk 3)
    if c["ff_factor1"] > 0:
        x = x + c["ff_factor1"] * ff("ff1", x)
        if not lnf:
            x = ln("ln3", x)
    return x


def stage_forward(x, w, st, new_st, cfg: dict, depth: int, training: bool, prefix: str = "at"):
    for i in range(depth):
        x = block_forward(x, w, st, new_st, f"{prefix}{i}", cfg, training)
    return x


attention_block = block_forward
attention_stage = stage_forward


def random_stage_weights(D: int, cfg: dict, depth: int, seed: int, prefix: str = "at"):
    """-> (flat trainable, flat state) float32: T.random_block_weights' rules (pos_bias_u / _v are kernels by their initializer, layers.py:343-356:
    drawn, not zero); moving statistics away from 0 / 1"""
    tr, nt = stage_specs(D, cfg, depth, prefix)
    rng = np.random.default_rng(seed + 7)
    st = [0.1 * rng.standard_normal(int(np.prod(s))) if n.endswith("moving_mean") else 1.0 + 0.3 * rng.random(int(np.prod(s))) for n, s in nt]
    w = T.random_block_weights(tr, seed)
    off = 0
    for n, s in tr:
        kk = int(np.prod(s))
        if n.endswith(("pos_bias_u", "pos_bias_v")):
            w[off:off + kk] = 0.3 * rng.standard_normal(kk)
        off += kk
    return w.astype(np.float32), (np.concatenate(st) if st else np.zeros(0)).astype(np.float32)


# ---- the reference's own two test configurations (modules_test.py:129-152, 295-317) with dropout_rate 0, and the GPU cases
REF_STAGE = {"depth": 3, "key_dim": 16, "n_head": 4, "kernel_size": 3, "ff_kernel_size": 3, "ff_multiplier": 2, "ff_factor0": 0, "ff_factor1": 0.5,
             "activation": "swish", "pos_encoding": "basic", "abs_pos_encoding": True, "layer_norm_in_front": True, "use_glu": False,
             "dropout_rate": 0}
REF_BLOCK = {"key_dim": 16, "n_head": 4, "kernel_size": 0, "ff_kernel_size": 3, "ff_multiplier": 2, "ff_factor0": 1, "ff_factor1": 0.5,
             "activation": "swish", "pos_encoding": "basic", "abs_pos_encoding": False, "layer_norm_in_front": False, "use_glu": True,
             "dropout_rate": 0}


def _cfg(**kw):
    return dict({"key_dim": 8, "n_head": 4, "kernel_size": 3, "ff_kernel_size": 3, "ff_multiplier": 2, "ff_factor0": 1, "ff_factor1": 0.5,
                 "dropout_rate": 0}, **kw)


STAGE_CASES = {"reference test_attention_stage": (2, 70, 32, 3, REF_STAGE), "reference test_attention_block": (2, 70, 32, 1, REF_BLOCK)}
for _lnf in (True, False):
    STAGE_CASES[f"relative lnf{int(_lnf)}"] = (2, 70, 32, 1, _cfg(layer_norm_in_front=_lnf))
for _k in (0, 3, 4):
    for _g in (True, False):
        STAGE_CASES[f"k{_k} glu{int(_g)}"] = (2, 70, 32, 1, _cfg(kernel_size=_k, use_glu=_g, layer_norm_in_front=_k == 4))
STAGE_CASES["ff_factor0 0"] = (2, 70, 32, 1, _cfg(ff_factor0=0, use_glu=True))
STAGE_CASES["use_bias"] = (2, 70, 32, 1, _cfg(use_bias=True, key_dim=16, n_head=2))
STAGE_CASES["stage depth 2"] = (2, 70, 32, 2, _cfg(depth=2, use_glu=True, layer_norm_in_front=True))

RELATTN_CASES = [(2, 1, 1, 8), (1, 2, 2, 8), (2, 63, 2, 16), (2, 64, 2, 24), (2, 65, 3, 8), (2, 130, 2, 64), (3, 100, 4, 16)]


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
    ns = torch.cat([new_st[n].detach().reshape(-1) for n, _ in nt]) if nt else torch.zeros(0, dtype=dtype)
    return {"x": x, "dy": dy, "w": w, "st": st, "out_train": yt.detach().numpy(), "out_eval": ye.numpy(), "new_state": ns.numpy(),
            "dx": gx.numpy(), "grad": gw.numpy(), "specs": (tr, nt)}


# ---- models.seldnet with a mother FIRST block and an attention SECOND block
def _depth(model_config: dict) -> int:
    if model_config["SECOND"] == "attention_stage":
        return int(model_config["SECOND_ARGS"]["depth"])
    if model_config["SECOND"] == "attention_block":
        return 1
    raise ValueError("attention_block_oracle restates attention_block / attention_stage as SECOND")


MODEL_INPUT = (2, 50, 64, 7)


def model_case(seldnet_config: dict, stage_first: dict) -> dict:
    """the composed model of the GPU train-step test: FIRST = one mother_block of tests/test_modules_gpu.STAGE_FIRST's shape with 8 + 8 filters,
    SECOND = a two-block attention_stage with relative positions, GLU, a depthwise module and both FF modules"""
    import copy
    cfg = copy.deepcopy(seldnet_config)
    first = dict(copy.deepcopy(stage_first), filters0=8, filters1=8)
    first.pop("depth", None)
    cfg["FIRST"], cfg["FIRST_ARGS"] = "mother_block", first
    cfg["SECOND"] = "attention_stage"
    cfg["SECOND_ARGS"] = {"depth": 2, "n_head": 4, "key_dim": 16, "kernel_size": 3, "ff_kernel_size": 3, "ff_multiplier": 0.5, "ff_factor0": 0.5,
                          "ff_factor1": 0.5, "use_glu": True, "dropout_rate": 0}
    return cfg


def variable_specs(model_config: dict, input_shape):
    gl = T._gru_less(model_config)
    tr, nt = M.variable_specs(gl, input_shape)
    shape = CF._first_out(model_config, input_shape)
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
    shape = CF._first_out(model_config, input_shape)
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
