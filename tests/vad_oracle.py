"""torch restatement (CPU, float64 unless a dtype is given) of the voice-activity model models.spectro_temporal_attention_based_VAD and of what
seld_amd/vad.py builds around it, written from the formulas of DESIGN.md section 3t.  A helper, not a test file: tests/test_vad_cpu.py checks
it against autograd and closed forms, tests/test_vad_gpu.py checks the device against it.

  variable_specs, random_weights     the model's variables in Keras creation order, and non-degenerate values for them
  gate_pool, gate_pool_backward      max over frequency pairs of a * sigmoid(b); the closed-form gradient with zeros at losers / the odd column
  temporal_attention (+ _backward)   head-fast reshape (column n = d H + h), softmax over t per head, score = softmax over t of the head sum
  temporal_attention_head_major      the same with column n = h D + d: what the kernel must NOT compute
  bce, bce_grad                      tf.keras.backend.binary_crossentropy on probabilities, meaned
  forward, train_step, adam_steps    the model, its summed loss and gradients (autograd), Adam
  dropout_masks                      the masks of the library's draws (oracle.seldnet_oracle.dropout_mask) at sites 0, 1 (pipe net), 2 (post net)
  margins                            the decision margins of a case: smallest pooled-pair gap and smallest relu |input|, each over its tensor's max
  seq_to_windows, windows_to_seq, predict_sequence      the irregular frame window, numpy
"""
from __future__ import annotations

import math

import numpy as np
import torch

from oracle import seldnet_oracle as O

DEFAULTS = {"T": 4, "Nc": 16, "fc": 3, "Np": 256, "Nt": 128, "H": 4, "dropout_rate": 0.5}
BN_EPS, BN_MOMENTUM = 1e-3, 0.99
BCE_EPS = float(np.float32(1e-7))
BCE_HI = float(np.float32(1.0) - np.float32(1e-7))      # the clip's upper end as fp32 holds it
SEED = 0x5e1d5e1d5e1d5e1d                               # the runtime's default dropout_seed
STREAM0 = 4096
REF_WINDOW = [0, 9, 18, 19, 20, 29, 38]                 # preprocess_window([-19, -10, -1, 0, 1, 10, 19])


def cfg_get(cfg: dict) -> dict:
    return dict(DEFAULTS, **cfg)


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


# ---------------------------------------------------------------- variables
def variable_specs(cfg: dict, input_shape):
    """-> (trainable, non-trainable) [(name, shape)]; input_shape (B, T, F, C) or (T, F, C)"""
    c = cfg_get(cfg)
    T, F, C = (int(v) for v in input_shape[-3:])
    tr, nt = [], []

    def bn(name, n):
        tr.extend([(f"{name}.gamma", (n,)), (f"{name}.beta", (n,))])
        nt.extend([(f"{name}.moving_mean", (n,)), (f"{name}.moving_variance", (n,))])

    def dense(name, k, n, bias=True):
        tr.append((f"{name}.kernel", (k, n)))
        if bias:
            tr.append((f"{name}.bias", (n,)))

    cin = C
    for i in range(c["T"]):
        f = c["Nc"] * 2 ** i
        for s in "ab":
            tr.extend([(f"sa{i}.conv_{s}.kernel", (c["fc"], c["fc"], cin, f)), (f"sa{i}.conv_{s}.bias", (f,))])
            bn(f"sa{i}.bn_{s}", f)
        cin, F = f, F // 2
    fin = F * cin
    for i, k in enumerate((fin, c["Np"])):
        dense(f"pipe{i}.dense", k, c["Np"])
        bn(f"pipe{i}.bn", c["Np"])
    dense("pipe_out", c["Np"], 1)
    for name in ("query", "key", "value"):
        dense(f"{name}.dense", c["Np"], c["Nt"], bias=False)
        bn(f"{name}.bn", c["Nt"])
    dense("post0.dense", c["Nt"], c["Np"])
    bn("post0.bn", c["Np"])
    dense("out", c["Np"], 1)
    return tr, nt


def random_weights(cfg: dict, input_shape, seed: int = 0):
    """-> (flat weights, flat state) fp32: every bias, gamma, beta and moving statistic non-trivial"""
    rng = np.random.default_rng(seed)
    tr, nt = variable_specs(cfg, input_shape)
    w = []
    for name, sh in tr:
        n = int(np.prod(sh))
        if name.endswith("gamma"):
            w.append(rng.uniform(0.5, 1.5, n))
        elif name.endswith(("beta", "bias")):
            w.append(rng.normal(0, 0.1, n))
        else:
            w.append(rng.normal(0, 1.0 / math.sqrt(int(np.prod(sh[:-1]))), n))
    st = [rng.uniform(0.5, 1.5, int(np.prod(sh))) if name.endswith("variance") else rng.normal(0, 0.1, int(np.prod(sh))) for name, sh in nt]
    return np.concatenate(w).astype(np.float32), np.concatenate(st).astype(np.float32)


def case_inputs(B: int, shape, seed: int):
    """-> x [B, T, F, C], y [B, T] in {0, 1}, fp32"""
    rng = np.random.default_rng(1000 + seed)
    return rng.standard_normal((B,) + tuple(shape)).astype(np.float32), (rng.random((B, shape[0])) < 0.5).astype(np.float32)


# ---------------------------------------------------------------- the three new pieces
def gate_pool(a, b):
    """a, b [..., W, C] -> (y [..., W // 2, C], win: the column of the pair that holds the maximum (the first of two equal ones), g)"""
    g = a * torch.sigmoid(b)
    Wo = g.shape[-2] // 2
    pairs = g[..., :2 * Wo, :].reshape(*g.shape[:-2], Wo, 2, g.shape[-1])
    win = (pairs[..., 1, :] > pairs[..., 0, :]).to(torch.int64)
    return torch.where(win.bool(), pairs[..., 1, :], pairs[..., 0, :]), win, g


def gate_pool_backward(a, b, win, dy):
    """the closed form: da = dy s, db = dy a s (1 - s) at the winner, 0 at the loser and in an odd last column"""
    s = torch.sigmoid(b)
    W, Wo = a.shape[-2], a.shape[-2] // 2
    route = torch.zeros_like(a)
    sel = torch.stack([(win == 0), (win == 1)], dim=-2).to(a.dtype) * dy.unsqueeze(-2)      # [..., Wo, 2, C]
    route[..., :2 * Wo, :] = sel.reshape(*a.shape[:-2], 2 * Wo, a.shape[-1])
    return route * s, route * a * s * (1 - s)


def _heads(t, H, head_fast=True):
    Nt = t.shape[-1]
    return t.reshape(*t.shape[:-1], Nt // H, H) if head_fast else t.reshape(*t.shape[:-1], H, Nt // H).transpose(-1, -2)


def temporal_attention(q, k, v, H: int, head_fast: bool = True):
    """q [B, Nt], k, v [B, T, Nt] before their sigmoid -> (y [B, T, Nt], score [B, T], P [B, T, H], s [B, T, H])"""
    Nt = q.shape[-1]
    sq, sk, sv = (_heads(torch.sigmoid(t), H, head_fast) for t in (q, k, v))      # [B, (T,) D, H]
    s = (sq[:, None] * sk).sum(dim=-2) / math.sqrt(Nt)                              # [B, T, H]
    P = torch.softmax(s, dim=1)
    y = sv * P[:, :, None, :]
    y = y.reshape(*k.shape) if head_fast else y.transpose(-1, -2).reshape(*k.shape)
    return y, torch.softmax(s.sum(dim=-1), dim=1), P, s


def temporal_attention_head_major(q, k, v, H: int):
    return temporal_attention(q, k, v, H, head_fast=False)


def temporal_attention_backward(q, k, v, H: int, dy, dscore):
    """the backward as the kernel evaluates it -> dq, dk, dv (pre-sigmoid)"""
    Nt = q.shape[-1]
    c = 1.0 / math.sqrt(Nt)
    _, score, P, _ = temporal_attention(q, k, v, H)
    sq, sk, sv = (_heads(torch.sigmoid(t), H) for t in (q, k, v))
    dyh = _heads(dy, H)
    dP = (dyh * sv).sum(dim=-2)
    dS = score * (dscore - (score * dscore).sum(dim=1, keepdim=True))
    ds = P * (dP - (P * dP).sum(dim=1, keepdim=True)) + dS[:, :, None]
    dsq = c * (ds[:, :, None, :] * sk).sum(dim=1)
    dsk = c * ds[:, :, None, :] * sq[:, None]
    dsv = dyh * P[:, :, None, :]
    back = lambda d, sg: (d * sg * (1 - sg)).reshape(*d.shape[:-2], Nt)
    return back(dsq, sq), back(dsk, sk), back(dsv, sv)


def bce(y, p):
    """mean over the elements of -(y log(pc + eps) + (1 - y) log(1 - pc + eps)), pc = clip(p, eps, 1 - eps)"""
    pc = torch.clamp(p, BCE_EPS, BCE_HI)
    return -(y * torch.log(pc + BCE_EPS) + (1 - y) * torch.log(1 - pc + BCE_EPS)).mean()


def bce_grad(y, p, weight=1.0):
    pc = torch.clamp(p, BCE_EPS, BCE_HI)
    g = ((1 - y) / (1 - pc + BCE_EPS) - y / (pc + BCE_EPS)) * (weight / p.numel())
    return torch.where((p < BCE_EPS) | (p > BCE_HI), torch.zeros_like(g), g)


# ---------------------------------------------------------------- the model
def batchnorm(z, gamma, beta, mm, mv, training: bool):
    """Keras BatchNormalization over every axis but the last -> (y, new moving mean, new moving variance)"""
    if not training:
        return (z - mm) * torch.rsqrt(mv + BN_EPS) * gamma + beta, mm, mv
    dims = tuple(range(z.dim() - 1))
    n = z.numel() // z.shape[-1]
    mean = z.mean(dim=dims)
    var = ((z - mean) ** 2).mean(dim=dims)
    with torch.no_grad():
        nm = mm * BN_MOMENTUM + mean * (1 - BN_MOMENTUM)
        nv = mv * BN_MOMENTUM + var * (n / max(n - 1, 1)) * (1 - BN_MOMENTUM)
    return (z - mean) * torch.rsqrt(var + BN_EPS) * gamma + beta, nm.detach(), nv.detach()


def conv2d_same(x, kernel, bias):
    """Conv2D(filters, k, padding='same') on NHWC x, HWIO kernel (odd or even k: TensorFlow pads the surplus behind)"""
    kh, kw = kernel.shape[0], kernel.shape[1]
    xp = torch.nn.functional.pad(x.permute(0, 3, 1, 2), ((kw - 1) // 2, kw - 1 - (kw - 1) // 2, (kh - 1) // 2, kh - 1 - (kh - 1) // 2))
    return torch.nn.functional.conv2d(xp, kernel.permute(3, 2, 0, 1), bias).permute(0, 2, 3, 1)


def dropout_masks(cfg: dict, B: int, T: int, step: int, seed: int = SEED, dtype=torch.float64):
    """-> {site: mask [B, T, Np]} of the library's draws at `step`, or None at rate 0"""
    c = cfg_get(cfg)
    rate = float(np.float32(c["dropout_rate"]))
    if rate == 0:
        return None
    return {site: O.dropout_mask((B, T, c["Np"]), rate, seed, STREAM0 + site, step, dtype) for site in range(3)}


def forward(cfg: dict, w: dict, st: dict, x, training: bool, masks=None, taps=None):
    """x [B, T, F, C] -> (out [B, T, 1], pipe [B, T, 1], score [B, T], new state); masks: dropout_masks(...) or None; taps (a dict) receives
    the decision tensors: 'gate{i}' (the gated tensor in front of pool i) and 'relu:{name}' (the relu inputs)"""
    c = cfg_get(cfg)
    new = dict(st)

    def bn(name, z):
        y, new[f"{name}.moving_mean"], new[f"{name}.moving_variance"] = batchnorm(z, w[f"{name}.gamma"], w[f"{name}.beta"], st[f"{name}.moving_mean"],
                                                                               st[f"{name}.moving_variance"], training)
        return y

    def dense_bn_relu(name, h, site):
        n = bn(f"{name}.bn", h @ w[f"{name}.dense.kernel"] + w[f"{name}.dense.bias"])
        if taps is not None:
            taps[f"relu:{name}"] = n
        h = torch.relu(n)
        return h * masks[site] if (training and masks is not None) else h

    h = x
    for i in range(c["T"]):
        a = bn(f"sa{i}.bn_a", conv2d_same(h, w[f"sa{i}.conv_a.kernel"], w[f"sa{i}.conv_a.bias"]))
        b = bn(f"sa{i}.bn_b", conv2d_same(h, w[f"sa{i}.conv_b.kernel"], w[f"sa{i}.conv_b.bias"]))
        h, _, g = gate_pool(a, b)
        if taps is not None:
            taps[f"gate{i}"] = g
    h = h.reshape(h.shape[0], h.shape[1], -1)
    for i in range(2):
        h = dense_bn_relu(f"pipe{i}", h, i)
    pipe = torch.sigmoid(h @ w["pipe_out.kernel"] + w["pipe_out.bias"])
    q = bn("query.bn", h.mean(dim=1) @ w["query.dense.kernel"])
    k = bn("key.bn", h @ w["key.dense.kernel"])
    v = bn("value.bn", h @ w["value.dense.kernel"])
    y, score, _, _ = temporal_attention(q, k, v, c["H"])
    h = dense_bn_relu("post0", y, 2)
    out = torch.sigmoid(h @ w["out.kernel"] + w["out.bias"])
    return out, pipe, score, new


def loss_fn(outs, y, loss_weights=(1.0, 1.0, 1.0)):
    return sum(wt * bce(y.reshape(o.shape), o) for wt, o in zip(loss_weights, outs))


def _flat(d: dict, specs):
    return np.concatenate([d[n].detach().numpy().reshape(-1) for n, _ in specs]) if specs else np.zeros(0)


def train_step(cfg: dict, input_shape, flat_w, flat_state, x, y, loss_weights=(1.0, 1.0, 1.0), masks=None, dtype=torch.float64, taps=None):
    """-> dict(out, pipe, score, loss, grad (flat), state (flat, after the step's moving-statistics update))"""
    tr, nt = variable_specs(cfg, input_shape)
    fw = torch.tensor(np.asarray(flat_w), dtype=dtype, requires_grad=True)
    st = O.unflatten(torch.tensor(np.asarray(flat_state), dtype=dtype), nt)
    if masks is not None:
        masks = {k: m.to(dtype) for k, m in masks.items()}
    out, pipe, score, new = forward(cfg, O.unflatten(fw, tr), st, torch.tensor(np.asarray(x), dtype=dtype), True, masks, taps)
    loss = loss_fn((out, pipe, score), torch.tensor(np.asarray(y), dtype=dtype), loss_weights)
    (g,) = torch.autograd.grad(loss, fw)
    return {"out": out.detach().numpy(), "pipe": pipe.detach().numpy(), "score": score.detach().numpy(), "loss": float(loss.detach()), "grad": g.numpy(),
            "state": _flat(new, nt)}


def infer(cfg: dict, input_shape, flat_w, flat_state, x, dtype=torch.float64):
    """inference with the moving statistics -> (out, pipe, score) numpy"""
    tr, nt = variable_specs(cfg, input_shape)
    w = O.unflatten(torch.tensor(np.asarray(flat_w), dtype=dtype), tr)
    st = O.unflatten(torch.tensor(np.asarray(flat_state), dtype=dtype), nt)
    with torch.no_grad():
        out, pipe, score, _ = forward(cfg, w, st, torch.tensor(np.asarray(x), dtype=dtype), False)
    return out.numpy(), pipe.numpy(), score.numpy()


def adam_steps(cfg: dict, input_shape, flat_w, flat_state, batches, lr=1e-3, b1=0.9, b2=0.999, eps=1e-7, masks=None):
    """Keras Adam over `batches` [(x, y)] from zero slots -> (weights, state, [loss per step]); masks: per step, or None"""
    w, st = np.asarray(flat_w, np.float64), np.asarray(flat_state, np.float64)
    m, v, losses = np.zeros_like(w), np.zeros_like(w), []
    for step, (x, y) in enumerate(batches, 1):
        r = train_step(cfg, input_shape, w, st, x, y, masks=None if masks is None else masks[step - 1])
        g = r["grad"]
        m, v = b1 * m + (1 - b1) * g, b2 * v + (1 - b2) * g * g
        w = w - lr * math.sqrt(1 - b2 ** step) / (1 - b1 ** step) * m / (np.sqrt(v) + eps)
        st = r["state"]
        losses.append(r["loss"])
    return w, st, losses


def margins(taps: dict):
    """-> (smallest |g[2w] - g[2w+1]| / max|g| over the gated tensors, smallest |relu input| / max|relu input| over the relu layers)"""
    pool, relu = [], []
    for name, t in taps.items():
        t = t.detach()
        if name.startswith("gate"):
            Wo = t.shape[-2] // 2
            p = t[..., :2 * Wo, :].reshape(*t.shape[:-2], Wo, 2, t.shape[-1])
            pool.append(float((p[..., 0, :] - p[..., 1, :]).abs().min() / t.abs().max()))
        else:
            relu.append(float(t.abs().min() / t.abs().max()))
    return min(pool), min(relu)


def zero_bias_names(cfg: dict, input_shape):
    """the biases in front of a BatchNormalization (their gradient is identically 0) -> {bias name: its layer's kernel name}"""
    tr, _ = variable_specs(cfg, input_shape)
    return {n: n[:-4] + "kernel" for n, _ in tr if n.endswith(".bias") and n not in ("pipe_out.bias", "out.bias")}


# ---------------------------------------------------------------- the irregular frame window
def seq_to_windows(seq, window):
    seq, window = np.asarray(seq), [int(v) for v in window]
    n = seq.shape[0] - max(window)
    return np.stack([seq[o:o + n] for o in window], axis=1)


def windows_to_seq(windows, window):
    windows, window = np.asarray(windows, np.float64), [int(v) for v in window]
    n, width = windows.shape[0], max(window)
    seq = np.zeros((n + width,) + windows.shape[2:])
    cnt = np.zeros(n + width)
    for i, o in enumerate(window):
        seq[o:o + n] += windows[:, i]
        cnt[o:o + n] += 1
    return seq / (cnt.reshape((-1,) + (1,) * (seq.ndim - 1)) + 1e-8)


def predict_sequence(cfg: dict, input_shape, flat_w, flat_state, x, window):
    """x [len, F, C] -> [len, 1]: windows, the model's `out` at inference, windows_to_seq"""
    out, _, _ = infer(cfg, input_shape, flat_w, flat_state, seq_to_windows(x, window))
    return windows_to_seq(out, window)


# ---------------------------------------------------------------- the cases tests/test_vad_gpu.py runs (tests/test_vad_cpu.py asserts their margins)
MARGIN = 1e-4                                           # decision margin a model case must keep on this oracle: ten times the fp32 error seen
SMALL_CFG = {"T": 2, "Nc": 4, "Np": 16, "Nt": 12, "H": 3, "dropout_rate": 0.0}
DEFAULT_CFG = dict(DEFAULTS, dropout_rate=0.0)
DEFAULT_INPUT = (4, 7, 80, 1)
# name -> (config, (B, T, F, C), seed, dropout step or None): seeds picked on this oracle so that both margins hold
MODEL_CASES = {
    "even": (SMALL_CFG, (4, 3, 10, 1), 3, None),
    "odd": (SMALL_CFG, (3, 5, 11, 1), 4, None),      # an odd frequency axis twice: 11 -> 5 -> 2
    "dropout": (dict(SMALL_CFG, dropout_rate=0.5), (4, 3, 10, 1), 3, 0),
}
ADAM_CASE = (SMALL_CFG, (4, 3, 10, 1), 3, 1e-3)         # config, input, seed, learning rate: two steps
GATE_CASES = [(3, 2, 1), (5, 5, 3), (7, 10, 4), (33, 6, 128), (257, 80, 16)]      # (rows, W, C)
TATTN_CASES = [(1, 1, 4, 1), (2, 3, 12, 3), (3, 7, 128, 4), (2, 64, 128, 1), (2, 5, 512, 8), (1, 64, 512, 512)]      # (B, T, Nt, H); the last: every limit at once
TATTN_SATURATED = ((2, 5, 24, 4), 40.0)                 # |k| up to ~ 150: sigmoid(k) is exactly 0 or 1 in fp32
BCE_CASES = [1, 7, 4097]


def model_case(name: str):
    """-> (cfg, input_shape, w, st, x, y, masks)"""
    cfg, shape, seed, step = MODEL_CASES[name]
    w, st = random_weights(cfg, shape, seed)
    x, y = case_inputs(shape[0], shape[1:], seed)
    return cfg, shape, w, st, x, y, (None if step is None else dropout_masks(cfg, shape[0], shape[1], step))


def gate_inputs(rows: int, W: int, C: int, seed: int = 0, margin: float = 1e-3):
    """-> a, b [rows, W, C], dy [rows, W // 2, C] fp32 with every pair's gap above margin * max|g|: the first of a near-tied pair is nudged"""
    rng = np.random.default_rng(seed)
    a, b = rng.standard_normal((rows, W, C)).astype(np.float32), rng.standard_normal((rows, W, C)).astype(np.float32)
    Wo = W // 2
    for _ in range(8):
        g = a.astype(np.float64) / (1 + np.exp(-b.astype(np.float64)))
        tied = np.abs(g[:, 0:2 * Wo:2] - g[:, 1:2 * Wo:2]) < margin * np.abs(g).max()
        if not tied.any():
            break
        a[:, 0:2 * Wo:2][tied] += np.float32(0.5)
    else:
        raise AssertionError("gate_inputs: pairs stay tied")
    return a, b, rng.standard_normal((rows, Wo, C)).astype(np.float32)


def tattn_inputs(B: int, T: int, Nt: int, H: int, seed: int = 0, k_scale: float = 1.0):
    """-> q [B, Nt], k, v, dy [B, T, Nt], dscore [B, T] fp32"""
    rng = np.random.default_rng(seed)
    n = lambda *sh: rng.standard_normal(sh).astype(np.float32)
    return n(B, Nt), n(B, T, Nt) * np.float32(k_scale), n(B, T, Nt), n(B, T, Nt), n(B, T)


def gate_reference(a, b, dy, dtype=torch.float64):
    t = lambda z: torch.tensor(np.asarray(z), dtype=dtype)
    y, win, _ = gate_pool(t(a), t(b))
    da, db = gate_pool_backward(t(a), t(b), win, t(dy))
    return y.numpy(), win.numpy(), da.numpy(), db.numpy()


def tattn_reference(q, k, v, dy, dscore, H: int, dtype=torch.float64):
    """-> dict y, score, P, dq, dk, dv (numpy)"""
    q, k, v, dy, dscore = (torch.tensor(np.asarray(z), dtype=dtype) for z in (q, k, v, dy, dscore))
    y, score, P, _ = temporal_attention(q, k, v, H)
    dq, dk, dv = temporal_attention_backward(q, k, v, H, dy, dscore)
    return {n: z.numpy() for n, z in (("y", y), ("score", score), ("P", P), ("dq", dq), ("dk", dk), ("dv", dv))}


def bce_inputs(n: int, seed: int = 0):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.02, 0.98, n).astype(np.float32), (rng.random(n) < 0.5).astype(np.float32)
