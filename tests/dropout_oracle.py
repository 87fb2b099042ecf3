"""fp64 restatement (torch, CPU) of the composed path's Dropout (seld_amd/modules.py::_Drop): the attention kernels'
probability masks and the three attention blocks' training forward with every Dropout of the reference (modules.py:392-402, 440-502,
566-628).  A helper, not a test file: tests/test_dropout_cpu.py pins the mask function, tests/test_dropout_gpu.py checks the device against it.
The reference draws from TensorFlow's generator, which nothing reproduces: it fixes the distribution, the library fixes the draws, and this
file restates them from oracle.seldnet_oracle.philox4x32_10 / dropout_mask.  Gradients come from autograd.

  attention_mask       M[b,h,n,m] = 0 where u < rate, else 1 / (1 - rate); u = (word >> 8) * 2^-24 of word (m & 3) of Philox4x32-10 at counter
                       (m >> 2, layer, step, (b H + h) S + n) under the key (seed lo, seed hi)
  dropped_attention    O = (softmax(scale Q K^T) * M) V per head; lse of the undropped logits
  Draws                one block's streams: layer = 4096 + 32 * (index of the block in its stage) + site, sites in reference order (STREAMS)
  transformer_block / conformer_block / attention_block, stage_forward      the blocks' training forward with masks
  transformer_model_train_step   models.seldnet with a transformer_encoder_stage as SECOND: one train step at a given dropout_step
"""
from __future__ import annotations

import math

import numpy as np
import torch

import attention_block_oracle as A
import conformer_oracle as CF
import transformer_oracle as T
from oracle import modules_oracle as M
from oracle import seldnet_oracle as O

SEED = 0x5e1d5e1d5e1d5e1d      # _Rt.dropout_seed's default
STREAM0 = 4096
# site -> the Dropout, in reference order
STREAMS = {
    "transformer": ("attention probabilities", "behind the attention", "FFN activation", "FFN output"),
    "conformer": ("first FFN activation", "first FFN output", "attention probabilities", "behind the attention", "behind the convolution module",
                  "second FFN activation", "second FFN output"),
    "attention": ("first FF activation", "first FF output", "attention probabilities", "behind the attention", "behind the depthwise tail",
                  "second FF activation", "second FF output"),
}


def rate32(rate) -> float:
    """the rate as the fp32 the library compares with"""
    return float(np.float32(rate))


def attention_mask(B: int, S: int, H: int, rate: float, seed: int, layer: int, step: int, dtype=torch.float64) -> torch.Tensor:
    """-> M [B, H, S(query), S(key)]"""
    S4 = (S + 3) // 4
    b, h, n, m4 = np.meshgrid(np.arange(B, dtype=np.uint64), np.arange(H, dtype=np.uint64), np.arange(S, dtype=np.uint64),
                              np.arange(S4, dtype=np.uint64), indexing="ij")
    elem = (b * np.uint64(H) + h) * np.uint64(S) + n
    assert int(elem.max()) < 2 ** 32
    words = O.philox4x32_10(m4, np.full(m4.shape, layer, np.uint64), np.full(m4.shape, step, np.uint64), elem, seed, seed >> 32)
    words = np.stack(words, axis=-1).reshape(B, H, S, 4 * S4)[..., :S]          # key m = 4 m4 + word
    u = (words >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    r = np.float32(rate)
    return torch.as_tensor((u >= r).astype(np.float64) / (1.0 - float(r)), dtype=dtype)


def dropped_attention(q, k, v, scale, mask):
    """q, k, v [B, S, H, d], mask [B, H, S, S] (None: no Dropout) -> (o [B, S, H, d], lse [B, H, S])"""
    logits = torch.einsum("bnhd,bmhd->bhnm", q, k) * scale
    p = torch.softmax(logits, dim=-1)
    if mask is not None:
        p = p * mask
    return torch.einsum("bhnm,bmhd->bnhd", p, v), torch.logsumexp(logits, dim=-1)


def attention_reference(q, k, v, do, scale, rate, seed, layer, step):
    """numpy [B, S, H, d] (fp32 values) -> [o [R, HD], lse [B, H, S], dq, dk, dv [R, HD]] in fp64"""
    B, S, H, d = q.shape
    tq, tk, tv = (torch.tensor(T.f32(a), requires_grad=True) for a in (q, k, v))
    mask = attention_mask(B, S, H, rate, seed, layer, step) if rate32(rate) > 0 else None
    o, lse = dropped_attention(tq, tk, tv, scale, mask)
    g = torch.autograd.grad((o * torch.tensor(T.f32(do))).sum(), (tq, tk, tv))
    return [o.detach().numpy().reshape(B * S, H * d), lse.detach().numpy()] + [t.numpy().reshape(B * S, H * d) for t in g]


class Draws:
    """one block's Dropout layers at one training step"""

    def __init__(self, rate: float, index: int, step: int, seed: int = SEED):
        self.rate, self.index, self.step, self.seed = rate32(rate), int(index), int(step), int(seed)

    def layer(self, site: int) -> int:
        return STREAM0 + 32 * self.index + site

    def drop(self, site: int, t):
        """Dropout of a [B, S, C] tensor: element e of the row-major tensor draws uniform e of the stream"""
        if self.rate == 0:
            return t
        return t * O.dropout_mask(tuple(t.shape), self.rate, self.seed, self.layer(site), self.step, t.dtype)

    def attention(self, site: int, q, k, v, scale):
        B, S, H, _ = q.shape
        mask = attention_mask(B, S, H, self.rate, self.seed, self.layer(site), self.step, q.dtype) if self.rate > 0 else None
        return dropped_attention(q, k, v, scale, mask)[0]


def cfg_rate(cfg: dict) -> float:
    return rate32(cfg.get("dropout_rate", 0.1))


def transformer_block(x, w, prefix: str, cfg: dict, dr: Draws):
    """modules.py:388-405"""
    act, dk, p = T.ACTS[cfg.get("activation", "relu")], int(cfg["key_dim"]), f"{prefix}.mha"
    proj = lambda part: torch.einsum("bsd,dhk->bshk", x, w[f"{p}.{part}.kernel"]) + w[f"{p}.{part}.bias"]
    o = dr.attention(0, proj("query"), proj("key"), proj("value"), 1.0 / math.sqrt(float(dk)))
    attn = torch.einsum("bshk,hkd->bsd", o, w[f"{p}.attention_output.kernel"]) + w[f"{p}.attention_output.bias"]
    x = T.layer_norm(x + dr.drop(1, attn), w[f"{prefix}.ln0.gamma"], w[f"{prefix}.ln0.beta"])
    ffn = dr.drop(2, act(O.conv1d_same(x, w[f"{prefix}.ffn0.kernel"], w[f"{prefix}.ffn0.bias"])))
    ffn = dr.drop(3, O.conv1d_same(ffn, w[f"{prefix}.ffn1.kernel"], w[f"{prefix}.ffn1.bias"]))
    return T.layer_norm(x + ffn, w[f"{prefix}.ln1.gamma"], w[f"{prefix}.ln1.beta"])


def _mha_ref(x, w, prefix: str, c: dict, dr: Draws, site: int):
    """layers.MultiHeadAttention_([x, x, x]) with its probabilities' Dropout (layers.py:253-257)"""
    q, k, v = (torch.einsum("bnd,hdo->bnho", x, w[f"{prefix}.{p}_kernel"]) for p in ("query", "key", "value"))
    if c["use_bias"]:
        q, k, v = q + w[f"{prefix}.q_bias"], k + w[f"{prefix}.k_bias"], v + w[f"{prefix}.v_bias"]
    o = dr.attention(site, q / math.sqrt(float(c["key_dim"])), k, v, 1.0)
    out = torch.einsum("bnhi,hio->bno", o, w[f"{prefix}.projection_kernel"])
    return out + w[f"{prefix}.projection_bias"] if c["use_bias"] else out


def conformer_block(x, w, st, new_st, prefix: str, cfg: dict, dr: Draws):
    """modules.py:432-506, training"""
    c = CF.cfg_get(cfg)
    act, ff = T.ACTS[c["activation"]], c["ffn_factor"]
    ln = lambda n, t: T.layer_norm(t, w[f"{prefix}.{n}.gamma"], w[f"{prefix}.{n}.beta"])
    dense = lambda n, t: t @ w[f"{prefix}.{n}.kernel"].reshape(-1, w[f"{prefix}.{n}.kernel"].shape[-1]) + w[f"{prefix}.{n}.bias"]
    ffn = lambda n, t, s0: dr.drop(s0 + 1, dense(n + "b", dr.drop(s0, act(dense(n + "a", t)))))
    x = x + ff * ffn("ffn0", ln("ln0", x), 0)
    if c["pos_encoding"] == "basic":
        x = x + torch.as_tensor(CF.pos_table(x.shape[1], x.shape[2])).to(x.dtype)
    x = x + dr.drop(3, _mha_ref(ln("ln1", x), w, f"{prefix}.mha", c, dr, 2))
    conv = CF.depthwise_conv1d(CF.glu(dense("pw0", ln("ln2", x))), w[f"{prefix}.dw.kernel"], w[f"{prefix}.dw.bias"])
    y, m, v = O.batchnorm(conv[:, :, None, :], w[f"{prefix}.bn.gamma"], w[f"{prefix}.bn.beta"], st[f"{prefix}.bn.moving_mean"],
                          st[f"{prefix}.bn.moving_variance"], True)
    new_st[f"{prefix}.bn.moving_mean"], new_st[f"{prefix}.bn.moving_variance"] = m, v
    conv = dr.drop(4, dense("pw1", T.ACTS["swish"](y[:, :, 0, :]))) + x
    return ln("ln4", x + ff * ffn("ffn1", ln("ln3", conv), 5))


def attention_block(x, w, st, new_st, prefix: str, cfg: dict, dr: Draws):
    """modules.py:553-634 with abs_pos_encoding, training"""
    c = A.cfg_get(cfg)
    assert c["abs_pos_encoding"]
    act, lnf, k = T.ACTS[c["activation"]], c["layer_norm_in_front"], c["kernel_size"]
    ln = lambda n, t: T.layer_norm(t, w[f"{prefix}.{n}.gamma"], w[f"{prefix}.{n}.beta"])
    conv = lambda n, t: A.conv1d_same(t, w[f"{prefix}.{n}.kernel"], w[f"{prefix}.{n}.bias"])
    ff = lambda n, t, s0: dr.drop(s0 + 1, conv(n + "b", dr.drop(s0, act(conv(n + "a", t)))))
    if c["ff_factor0"] > 0:
        x = x + c["ff_factor0"] * ff("ff0", x, 0)
        if not lnf:
            x = ln("ln0", x)
    attn = ln("ln1", x) if lnf else x
    if c["pos_encoding"] == "basic":
        x = x + torch.as_tensor(CF.pos_table(x.shape[1], x.shape[2])).to(x.dtype)
    x = dr.drop(3, _mha_ref(attn, w, f"{prefix}.mha", c, dr, 2)) + x
    if not lnf:
        x = ln("ln1", x)
    cv = x
    if c["use_glu"]:
        cv = CF.glu(conv("pw0", ln("ln2", cv) if lnf else cv))
    if k > 0:
        if lnf and not c["use_glu"]:
            cv = ln("ln2", cv)
        cv = CF.depthwise_conv1d(cv, w[f"{prefix}.dw.kernel"], w[f"{prefix}.dw.bias"])
        y, m, v = O.batchnorm(cv[:, :, None, :], w[f"{prefix}.bn.gamma"], w[f"{prefix}.bn.beta"], st[f"{prefix}.bn.moving_mean"],
                              st[f"{prefix}.bn.moving_variance"], True)
        new_st[f"{prefix}.bn.moving_mean"], new_st[f"{prefix}.bn.moving_variance"] = m, v
        x = x + dr.drop(4, conv("pw1", T.ACTS["swish"](y[:, :, 0, :])))
        if not lnf:
            x = ln("ln2", x)
    else:
        x = cv
    if c["ff_factor1"] > 0:
        x = x + c["ff_factor1"] * ff("ff1", x, 5)
        if not lnf:
            x = ln("ln3", x)
    return x


KINDS = {"transformer": ("tf", lambda x, w, st, ns, p, cfg, dr: transformer_block(x, w, p, cfg, dr), lambda D, cfg, depth: (T.stage_specs(D, cfg, depth), [])),
         "conformer": ("cf", conformer_block, CF.stage_specs), "attention": ("at", attention_block, A.stage_specs)}


def stage_forward(kind: str, x, w, st, new_st, cfg: dict, depth: int, step: int, seed: int = SEED):
    """the training forward of `depth` blocks at dropout step `step`"""
    prefix, block, _ = KINDS[kind]
    for i in range(depth):
        x = block(x, w, st, new_st, f"{prefix}{i}", cfg, Draws(cfg_rate(cfg), i, step, seed))
    return x


def stage_reference(kind: str, B, S, D, depth, cfg, seed, step, dtype=torch.float64):
    """-> dict: x, dy, w, st (numpy inputs), out (the training forward at dropout step `step`), dx, grad, specs"""
    tr, nt = KINDS[kind][2](D, cfg, depth)
    if kind == "transformer":
        w, st = T.random_block_weights(tr, seed), np.zeros(0, np.float32)
    else:
        w, st = (CF if kind == "conformer" else A).random_stage_weights(D, cfg, depth, seed)
    rng = np.random.default_rng(seed)
    x, dy = T.f32(rng.standard_normal((B, S, D))), T.f32(rng.standard_normal((B, S, D)))
    fw = torch.tensor(w, dtype=dtype, requires_grad=True)
    xt = torch.tensor(x, dtype=dtype, requires_grad=True)
    sd = O.unflatten(torch.tensor(st, dtype=dtype), nt)
    yt = stage_forward(kind, xt, O.unflatten(fw, tr), sd, dict(sd), cfg, depth, step)
    gw, gx = torch.autograd.grad((yt * torch.tensor(dy, dtype=dtype)).sum(), (fw, xt))
    return {"x": x, "dy": dy, "w": w, "st": st, "out": yt.detach().numpy(), "dx": gx.numpy(), "grad": gw.numpy(), "specs": (tr, nt)}


def transformer_model_train_step(model_config: dict, input_shape, flat_w, flat_state, x, y_sed, y_doa, *, dropout_step: int, seed: int = SEED,
                                 doa_loss="MSE", loss_weight=(1.0, 1000.0), dtype=torch.float64):
    """transformer_oracle.train_step with the SECOND stage's Dropouts drawing at `dropout_step` -> dict(sed, doa, sloss, dloss, grad)"""
    tr, nt = T.variable_specs(model_config, input_shape)
    fw = torch.tensor(np.asarray(flat_w), dtype=dtype, requires_grad=True)
    w = O.unflatten(fw, tr)
    st = O.unflatten(torch.tensor(np.asarray(flat_state), dtype=dtype), nt)
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype)
    new_st = dict(st)
    h = t(x)
    for d, cfg in enumerate(M.first_configs(model_config)):
        h = M.mother_block_forward(cfg, w, st, new_st, h, True, f"mb{d}")
    h = h.reshape(h.shape[0], h.shape[1], -1)
    h = stage_forward("transformer", h, w, st, new_st, model_config["SECOND_ARGS"], T._depth(model_config), dropout_step, seed)
    sp = M._tail_spec(T._gru_less(model_config))
    outs = []
    for head, units, act, hact in (("sed", sp.sed_units, torch.sigmoid, T.ACTS[sp.sed_dense_act]), ("doa", sp.doa_units, torch.tanh, T.ACTS[sp.doa_dense_act])):
        a = h
        for j in range(len(units)):
            a = hact(a @ w[f"{head}.dense{j}.kernel"][0] + w[f"{head}.dense{j}.bias"])
        outs.append(act(a @ w[f"{head}.out.kernel"] + w[f"{head}.out.bias"]))
    obj, sloss, dloss = O.losses_and_objective(outs[0], outs[1], t(y_sed), t(y_doa), doa_loss, loss_weight)
    (g,) = torch.autograd.grad(obj, fw)
    return {"sed": outs[0].detach().numpy(), "doa": outs[1].detach().numpy(), "sloss": sloss.detach().numpy(), "dloss": dloss.detach().numpy(),
            "grad": g.numpy()}
