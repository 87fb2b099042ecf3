"""fp64 restatement of the reference's models.vad_architecture (models.py:81-102) and of its head's kernels (seld_amd/csrc/vadarch.hip).  A
helper, not a test file: tests/test_vadarch_cpu.py pins its pieces, tests/test_vadarch_gpu.py checks the device against it.

  head_reference         numpy fp64: p = sigmoid(x w + b), the mean binary cross-entropy of seld_vad_bce (clip to [1e-7, 1 - 1e-7], + 1e-7 inside
                         the logarithms, the derivative 0 where the clip is active), dz = dp p (1 - p), dx = dz w^T, dw = x^T dz, db = sum dz
  forward / train_step   the model (torch fp64, gradients from autograd): the optional flatten, the BLOCK* chain sorted as strings —
                         mother_block / mother_stage from oracle/modules_oracle.py, simple_dense_block / simple_dense_stage / identity_block
                         as the reference writes them (Dense (D, u) on a 2-D tensor, Conv1D (k, D, u) on a 3-D one, simple_dense_stage's
                         dense_activation = model_config.get('activation')) with Dropout behind each activation from tests/dropout_oracle.py's
                         Draws (block index = the blocks built in front, site = the layer) — force_1d_inputs, Dense(last_unit, sigmoid), squeeze
  relu_margin            the smallest |pre-activation| of every relu of a training forward over the largest: a case whose gradients are
                         compared keeps it above MARGIN, so that fp32 decides every relu as fp64 does
"""
from __future__ import annotations

import copy
import functools

import numpy as np
import torch

import dropout_oracle as DO
import transformer_oracle as T
from oracle import modules_oracle as M
from oracle import seldnet_oracle as O

f32 = T.f32
EPS = float(np.float32(1e-7))
HI = float(np.float32(1.0) - np.float32(1e-7))      # the clip's upper end as fp32 holds it
SEED = DO.SEED
MARGIN = 1e-4      # relative decision margin of a model case: ten times the fp32 error of a pre-activation at these sizes (K <= 560 terms)

# (rows, D, U): one element; D % 4 != 0; a full 64-row group and one past it; every U; D past a lane group's 256 columns; the nas_vad head
# on the data (1792 = 256 windows of 7 frames); the widest D of the search space (80 * 256)
HEAD_CASES = [(1, 1, 1), (7, 3, 1), (63, 4, 7), (64, 63, 1), (65, 64, 8), (65, 65, 7), (5, 257, 1), (1792, 80, 1), (9, 20480, 1)]
# past the cap of 1024 row chunks: 35000 rows run 1000 chunks of 35 rows and 24 that hold none; 33600 rows fill 1019 of them — the batch a
# model built for 35000 rows may meet, on the scratch of 35000
CAPPED_CASES = [(35000, 3, 2), (33600, 3, 2)]
SATURATED_LOGIT = 40.0


# ---------------------------------------------------------------- the head
def head_inputs(rows: int, D: int, U: int, seed: int = 0):
    """-> x [rows, D], w [D, U], b [U], y [rows, U] (0 / 1), fp32 values as float64; logits of order 1"""
    rng = np.random.default_rng([rows, D, U, seed])
    x = f32(rng.standard_normal((rows, D)))
    w = f32(rng.standard_normal((D, U)) * (1.5 / np.sqrt(D)))
    b = f32(0.3 * rng.standard_normal(U))
    y = (rng.random((rows, U)) < 0.5).astype(np.float64)
    return x, w, b, y


def head_forward(x, w, b):
    return 1.0 / (1.0 + np.exp(-(x @ w + b)))


def head_backward(x, w, p, y, weight: float = 1.0):
    """from the probabilities the device holds (fp32 values): -> (loss, dz, dx, dw, db)"""
    n = p.size
    pc = np.clip(p, EPS, HI)
    a, q = pc + EPS, 1.0 - pc + EPS
    loss = weight / n * float(-(y * np.log(a) + (1.0 - y) * np.log(q)).sum())
    dp = np.where((p < EPS) | (p > HI), 0.0, weight / n * ((1.0 - y) / q - y / a))
    dz = dp * p * (1.0 - p)
    return loss, dz, dz @ w.T, x.T @ dz, dz.sum(axis=0)


def head_reference(x, w, b, y, weight: float = 1.0):
    """-> dict(p, loss, dz, dx, dw, db), the backward from the fp64 p"""
    p = head_forward(x, w, b)
    loss, dz, dx, dw, db = head_backward(x, w, p, y, weight)
    return {"p": p, "loss": loss, "dz": dz, "dx": dx, "dw": dw, "db": db}


def saturated_inputs(rows: int = 6, D: int = 8, U: int = 2):
    """logits of exactly +-SATURATED_LOGIT in the first two rows: x = (1, 0, ...) against w[0] = +-40, b = 0"""
    x, w, b, y = head_inputs(rows, D, U, seed=3)
    b[:] = 0.0
    w[0] = [SATURATED_LOGIT, -SATURATED_LOGIT][:U]
    x[:2] = 0.0
    x[:2, 0] = 1.0
    x[2:, 0] = f32(0.01 * x[2:, 0])      # the other rows stay inside the clip
    y[0], y[1] = 1.0, 0.0
    return x, w, b, y


# ---------------------------------------------------------------- the model
DENSE = ("simple_dense_block", "simple_dense_stage", "identity_block")
MOTHER = ("mother_block", "mother_stage")


def blocks_of(model_config: dict):
    return sorted(k for k in model_config if k.startswith("BLOCK") and not k.endswith("_ARGS"))


def _dense_args(kind: str, args: dict) -> dict:
    a = copy.deepcopy(args)
    if kind == "simple_dense_stage":           # modules.py:86-103
        a["units"] = [a["units"]] * a["depth"]
        a["dense_activation"] = a.get("activation", None)
    elif kind == "identity_block":             # modules.py:639-642
        a = {"units": []}
    return a


def _mother_cfgs(kind: str, args: dict):
    return M.stage_configs(args) if kind == "mother_stage" else [copy.deepcopy(args)]


def walk(model_config: dict, input_shape):
    """-> (trainable, state, plan, output shape without the batch); plan: [('mother', cfg, prefix) | ('dense', args, prefix, block index, flat)]"""
    Wn, Fq, Ch = (int(v) for v in input_shape[-3:])
    flatten, U = bool(model_config.get("flatten", True)), int(model_config.get("last_unit", 1))
    tr, nt, plan, built = [], [], [], 0
    shape, D = (Wn, Fq, Ch), (Wn * Fq * Ch if flatten else None)
    for i, key in enumerate(blocks_of(model_config)):
        kind, args = model_config[key], model_config[f"{key}_ARGS"]
        if kind in MOTHER:
            assert not flatten and D is None
            for d, c in enumerate(_mother_cfgs(kind, args)):
                t, n, shape = M.mother_block_plan(c, shape, f"b{i}.mb{d}")
                tr, nt = tr + t, nt + n
                plan.append(("mother", c, f"b{i}.mb{d}"))
                built += 1
        else:
            assert kind in DENSE, kind
            a = _dense_args(kind, args)
            D = shape[1] * shape[2] if D is None else D
            k = int(a.get("kernel_size", 1))
            for j, u in enumerate(a["units"]):
                tr += [(f"b{i}.dense{j}.kernel", (D, int(u)) if flatten else (k, D, int(u))), (f"b{i}.dense{j}.bias", (int(u),))]
                D = int(u)
            plan.append(("dense", a, f"b{i}", built, flatten))
            built += 1
    D = shape[1] * shape[2] if D is None else D
    tr += [("out.kernel", (D, U)), ("out.bias", (U,))]
    lead = () if flatten else (shape[0],)
    return tr, nt, plan, lead + (() if U == 1 else (U,))


def variable_specs(model_config: dict, input_shape):
    return walk(model_config, input_shape)[:2]


def random_weights(model_config: dict, input_shape, seed: int = 0):
    """glorot-uniform kernels, every bias / gamma / beta perturbed (T.random_block_weights); moving statistics away from 0 / 1"""
    tr, nt = variable_specs(model_config, input_shape)
    rng = np.random.default_rng(seed + 7)
    st = [0.1 * rng.standard_normal(int(np.prod(s))) if n.endswith("moving_mean") else 1.0 + 0.3 * rng.random(int(np.prod(s))) for n, s in nt]
    return T.random_block_weights(tr, seed), (np.concatenate(st) if st else np.zeros(0)).astype(np.float32)


def forward(model_config: dict, input_shape, w, st, x, training: bool, step=None, seed: int = SEED, taps=None):
    """x [B, Wn, F, C] -> (prediction, new state).  step: the dropout_step whose masks a training forward draws (None: no Dropout, which is
    also inference); taps: a list that receives every relu's pre-activation"""
    _, _, plan, _ = walk(model_config, input_shape)
    new_st = dict(st)
    relu = M.ACTS["relu"]

    def tapped(t):
        if taps is not None:
            taps.append(t.detach())
        return relu(t)

    acts = dict(M.ACTS, relu=tapped)
    h = x.reshape(x.shape[0], -1) if model_config.get("flatten", True) else x
    M.ACTS["relu"] = tapped
    try:
        for item in plan:
            if item[0] == "mother":
                h = M.mother_block_forward(item[1], w, st, new_st, h, training, item[2])
                continue
            _, a, prefix, index, flat = item
            if h.dim() == 4:
                h = h.reshape(h.shape[0], h.shape[1], -1)      # layers.force_1d_inputs (layers.py:41-47)
            dr = DO.Draws(a.get("dropout_rate", 0) or 0, index, step or 0, seed)
            for j in range(len(a["units"])):
                kern, bias = w[f"{prefix}.dense{j}.kernel"], w[f"{prefix}.dense{j}.bias"]
                h = acts[a.get("dense_activation", None)](h @ kern + bias if flat else O.conv1d_same(h, kern, bias))
                if training and step is not None:
                    h = dr.drop(j, h)
    finally:
        M.ACTS["relu"] = relu
    if h.dim() == 4:
        h = h.reshape(h.shape[0], h.shape[1], -1)
    p = torch.sigmoid(h @ w["out.kernel"] + w["out.bias"])
    return (p[..., 0] if p.shape[-1] == 1 else p), new_st


def bce(y, p):
    pc = torch.clamp(p, EPS, HI)
    return -(y * torch.log(pc + EPS) + (1 - y) * torch.log(1 - pc + EPS)).mean()


def train_step(model_config: dict, input_shape, flat_w, flat_state, x, y, step=None, seed: int = SEED, taps=None, dtype=torch.float64):
    """-> dict(pred, loss, grad, new_state), numpy"""
    tr, nt = variable_specs(model_config, input_shape)
    fw = torch.tensor(np.asarray(flat_w), dtype=dtype, requires_grad=True)
    sd = O.unflatten(torch.tensor(np.asarray(flat_state), dtype=dtype), nt)
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype)
    p, new_st = forward(model_config, input_shape, O.unflatten(fw, tr), sd, t(x), True, step, seed, taps)
    loss = bce(t(y), p)
    (g,) = torch.autograd.grad(loss, fw)
    ns = torch.cat([new_st[n].detach().reshape(-1) for n, _ in nt]) if nt else torch.zeros(0, dtype=dtype)
    return {"pred": p.detach().numpy(), "loss": float(loss.detach()), "grad": g.numpy(), "new_state": ns.numpy()}


def infer(model_config: dict, input_shape, flat_w, flat_state, x, dtype=torch.float64):
    tr, nt = variable_specs(model_config, input_shape)
    with torch.no_grad():
        p, _ = forward(model_config, input_shape, O.unflatten(torch.tensor(np.asarray(flat_w), dtype=dtype), tr),
                       O.unflatten(torch.tensor(np.asarray(flat_state), dtype=dtype), nt), torch.as_tensor(np.asarray(x), dtype=dtype), False)
    return p.numpy()


def adam_steps(model_config: dict, input_shape, flat_w, flat_state, batches, lr=1e-3):
    """train.Adam from zero slots over `batches` (rate-0 Dropout) -> (weights, state, losses)"""
    w = torch.tensor(np.asarray(flat_w), dtype=torch.float64)
    m, v, st, losses = torch.zeros_like(w), torch.zeros_like(w), np.asarray(flat_state), []
    for i, (x, y) in enumerate(batches):
        r = train_step(model_config, input_shape, w.numpy(), st, x, y)
        w, m, v = O.adam_update(w, torch.tensor(r["grad"]), m, v, i + 1, lr=lr)
        st = r["new_state"]
        losses.append(r["loss"])
    return w.numpy(), st, losses


def relu_margin(taps) -> float:
    """min over the relus of min|pre| / max|pre| (1 without a relu)"""
    return min([float(t.abs().min() / t.abs().max()) for t in taps], default=1.0)


def zero_bias_names(model_config: dict, input_shape):
    """convolution biases in front of a training-mode BatchNormalization: their gradient is zero by mathematics"""
    tr, _ = variable_specs(model_config, input_shape)
    return {n for n, _ in tr if ".mb" in n and n.endswith(".bias") and ".s2_" not in n and ".se" not in n}


# ---------------------------------------------------------------- the configurations of the tests
MOTHER_B = {"depth": 2, "filters0": 0, "filters1": 6, "filters2": 4, "kernel_size0": 0, "kernel_size1": 3, "kernel_size2": 1, "connect0": [1],
            "connect1": [1, 0], "connect2": [0, 0, 1], "strides": [1, 2]}      # the skips p1_0 (strided) and p2_2 are projections
CFG_A = {"flatten": True, "last_unit": 7, "BLOCK0": "simple_dense_stage", "BLOCK0_ARGS": {"depth": 2, "units": 24, "activation": "relu"}}
CFG_B = {"flatten": False, "last_unit": 1, "BLOCK0": "mother_stage", "BLOCK0_ARGS": MOTHER_B,
         "BLOCK1": "simple_dense_stage", "BLOCK1_ARGS": {"depth": 1, "units": 12, "activation": "relu"}}
CFG_A_DROP = dict(CFG_A, BLOCK0_ARGS=dict(CFG_A["BLOCK0_ARGS"], dropout_rate=0.5))
MODEL_CASES = {"a": (CFG_A, (3, 7, 80, 1)), "b": (CFG_B, (3, 7, 10, 1)), "a_drop": (CFG_A_DROP, (3, 7, 80, 1))}
# the two configurations of models_test.py::test_vad_architecture
REF_TEST_CONFIGS = [
    {"flatten": True, "last_unit": 7, "BLOCK0": "simple_dense_stage",
     "BLOCK0_ARGS": {"depth": 2, "units": 512, "dense_activation": "relu", "dropout_rate": 0.5}},
    {"flatten": False, "last_unit": 1, "BLOCK0": "simple_dense_stage",
     "BLOCK0_ARGS": {"depth": 2, "units": 512, "dense_activation": "relu", "dropout_rate": 0.5}},
]


def case_inputs(model_config: dict, input_shape, seed: int):
    """-> (x ~ N(0.3, 1): a mean the BatchNormalizations have to remove; y 0 / 1 of the prediction's shape), fp32 values"""
    rng = np.random.default_rng(seed)
    out = walk(model_config, input_shape)[3]
    x = f32(0.3 + rng.standard_normal(tuple(input_shape)))
    return x, (rng.random((input_shape[0],) + out) < 0.5).astype(np.float64)


@functools.lru_cache(maxsize=None)
def model_case(name: str):
    """-> (config, input shape, weights, state, x, y, seed): the first seed whose training forward keeps every relu MARGIN away from 0"""
    cfg, shape = MODEL_CASES[name]
    for seed in range(64):
        w, st = random_weights(cfg, shape, seed)
        x, y = case_inputs(cfg, shape, seed)
        taps = []
        train_step(cfg, shape, w, st, x, y, taps=taps)
        if relu_margin(taps) >= MARGIN:
            return cfg, shape, w, st, x, y, seed
    raise AssertionError(f"{name}: no seed keeps the relu margin")
