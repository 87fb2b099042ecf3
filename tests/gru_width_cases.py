"""Cases of the any-width GRU recurrence (seld_rnn_gruw_fwd / _bwd, seld_amd/csrc/gru_w.hip) shared by tests/test_gru_width_cpu.py and
tests/test_gru_width_gpu.py: width-taking forms of rnn_oracle.recurrence_inputs / gru_pieces (those hard-code 128 units), the case lists —
derived from what seld_rnn_gruw_plan reports, so that they bracket the kernels' boundaries without naming them — and the two model
configurations.  The fp64 references come from rnn_oracle.gru_reference (width-generic), computed once per case and shared."""
import ctypes as C
import functools
import math

import numpy as np
import torch

import conv_temporal_oracle as CT
import rnn_oracle as R

FP32_MARGIN = 5e-5      # the rule of tests/test_rnn_cpu.py: a plain fp32 evaluation of every GPU case stays this close to fp64
SEARCH_UNITS = [4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256]      # nas_seldnet.search_space_1d
EXTRA_UNITS = [1, 3, 100, 127, 129, 255]
MAX_UNITS = 256
SATURATED = (2, 17, 8.0)      # B, S, the factor on gx: |z| far in the gates' flat ends (rnn_oracle.GRU_SATURATED)


def gruw_plan(u: int):
    """-> ((form, clips per workgroup, forward chunk, backward chunk), number of forms) from the library; no device needed"""
    from seld_amd import _lib
    out = (C.c_int32 * 4)()
    n = _lib.load().seld_rnn_gruw_plan(int(u), out)
    assert n >= 1, (u, n)
    return tuple(int(v) for v in out), n


@functools.lru_cache(maxsize=None)
def widths():
    """every search-space value, the odd ones of EXTRA_UNITS, and both sides of every u where the reported form or tile changes"""
    ws = set(SEARCH_UNITS) | set(EXTRA_UNITS)
    for u in range(2, MAX_UNITS + 1):
        if gruw_plan(u)[0][:2] != gruw_plan(u - 1)[0][:2]:
            ws |= {u - 1, u}
    return sorted(ws)


def s_values(u: int):
    (_, _, fc, bc), _ = gruw_plan(u)
    s = {1, 2, 60}
    for c in (fc, bc):
        s |= {c - 1, c, c + 1, 2 * c + 1}
    return sorted(v for v in s if v >= 1)


def b_values(u: int):
    t = gruw_plan(u)[0][1]
    return sorted({1} | ({t - 1, t, t + 1} if t > 1 else {1, 3}))


def cases(u: int):
    """[(B, S)] of width u: the product of its B and S lists"""
    return [(b, s) for b in b_values(u) if b >= 1 for s in s_values(u)]


def one_width_per_form():
    """{form: a width}: the search-space width in the middle of each form's range"""
    by = {}
    for u in SEARCH_UNITS:
        by.setdefault(gruw_plan(u)[0][0], []).append(u)
    return {f: us[len(us) // 2] for f, us in sorted(by.items())}


def inputs(B: int, S: int, u: int, scale: float = 1.0, seed: int = 0):
    """-> dict of float32 numpy: gx [2][B,S,3u], U [2][u,3u], brec [2][3u], dh [2][B,S,u]; index 0 = forward, 1 = backward direction"""
    rng = np.random.default_rng([B, S, u, seed])
    return {"gx": R.f32(scale * rng.standard_normal((2, B, S, 3 * u))), "U": R.f32(rng.standard_normal((2, u, 3 * u)) / math.sqrt(u)),
            "brec": R.f32(0.1 * rng.standard_normal((2, 3 * u))), "dh": R.f32(rng.standard_normal((2, B, S, u)))}


@functools.lru_cache(maxsize=None)
def reference(B: int, S: int, u: int, scale: float = 1.0, fp32: bool = False):
    """(inputs, rnn_oracle.gru_reference of them in fp64 — or, fp32, in plain float32)"""
    ins = inputs(B, S, u, scale)
    return ins, R.gru_reference(ins, torch.float32 if fp32 else torch.float64)


def pieces(got, ref, u: int):
    """rnn_oracle.gru_pieces at width u: h whole, dgx / dgh by their z | r | h thirds, saved [B,S,u,4] by its four planes -> [(name, got, ref)]"""
    res = []
    for k, arrs in got.items():
        for i, a in enumerate(arrs):
            a = np.asarray(a)
            if k == "h":
                res.append((f"h[{i}]", a, ref["h"][i]))
            elif k in ("dgx", "dgh"):
                for g, gate in enumerate("zrh"):
                    res.append((f"{k}[{i}].{gate}", a[..., g * u:(g + 1) * u], ref[k][i][..., g * u:(g + 1) * u]))
            elif k == "saved":
                a = a.reshape(ref["z"][i].shape + (4,))
                for g, plane in enumerate(R.GRU_SAVED):
                    res.append((f"saved[{i}].{plane}", a[..., g], ref[plane][i]))
            else:
                raise KeyError(k)
    for name, a, b in res:
        assert a.shape == np.asarray(b).shape, f"{name}: {a.shape} against {np.asarray(b).shape}"
    return res


def compare(tag, got, ref, u: int, tol: float):
    """helpers.check on every piece; every piece is measured and printed before the failures are raised together"""
    from helpers import check
    bad = []
    for name, a, b in pieces(got, ref, u):
        try:
            check(f"{tag} {name}", a, b, tol)
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, "; ".join(bad)


def as_kernel_outputs(ref):
    """an oracle result in the kernels' layout: {h, saved [B,S,u,4], dgx, dgh} per direction"""
    return {"h": ref["h"], "saved": [R.gru_saved(ref, i) for i in range(len(ref["h"]))], "dgx": ref["dgx"], "dgh": ref["dgh"]}


# ---------------------------------------------------------------- blocks through seld_amd.modules
# name -> (kind, B, S, D, depth (None: a block), config)
BLOCK_CASES = {f"RNN_block u24 {m}": ("RNN_block", 3, 9, 20, None, {"units": 24, "rnn_type": "GRU", "merge_mode": m, "dropout_rate": 0.0})
               for m in R.MERGES}
BLOCK_CASES["RNN_block u24 one direction"] = ("RNN_block", 3, 9, 20, None,
                                              {"units": 24, "rnn_type": "GRU", "bidirectional": False, "merge_mode": None, "dropout_rate": 0.0})
GRU_BLOCK_CASE = (3, 9, 20, {"units": [12, 128, 5], "dropout_rate": 0.0})      # B, S, D, bidirectional_GRU_block's config


def gru_block_specs(D: int, units, prefix: str = "gru"):
    tr = []
    for i, u in enumerate(units):
        tr += R.block_specs(D, {"units": u}, f"{prefix}{i}")
        D = u
    return tr


def gru_block_reference(B, S, D, cfg, seed, dtype=torch.float64):
    """bidirectional_GRU_block with a width per layer (merge 'mul') -> dict as rnn_oracle.stage_reference's"""
    from oracle import seldnet_oracle as O
    import transformer_oracle as T
    units = [int(u) for u in cfg["units"]]
    tr = gru_block_specs(D, units)
    w = T.random_block_weights(tr, seed)
    rng = np.random.default_rng(seed)
    x, dy = R.f32(rng.standard_normal((B, S, D))), R.f32(rng.standard_normal((B, S, units[-1])))
    fw = torch.tensor(w, dtype=dtype, requires_grad=True)
    xt = torch.tensor(x, dtype=dtype, requires_grad=True)
    ws, y = O.unflatten(fw, tr), xt
    for i, u in enumerate(units):
        y = R.block_forward(y, ws, {"units": u}, f"gru{i}")
    gw, gx = torch.autograd.grad((y * torch.tensor(dy, dtype=dtype)).sum(), (fw, xt))
    return {"x": x, "dy": dy, "w": w, "out": y.detach().numpy(), "dx": gx.numpy(), "grad": gw.numpy(), "specs": tr}


# ---------------------------------------------------------------- models
CONFIG_A = {
    "n_classes": 3, "filters": 4, "first_kernel_size": 3, "first_pool_size": [2, 2],
    "BLOCK0": "bidirectional_GRU_stage", "BLOCK0_ARGS": {"depth": 2, "units": 12},
    "BLOCK1": "RNN_stage", "BLOCK1_ARGS": {"depth": 1, "units": 6, "rnn_type": "GRU", "merge_mode": "concat"},
    "SED": "bidirectional_GRU_stage", "SED_ARGS": {"depth": 1, "units": 5},
    "DOA": "RNN_block", "DOA_ARGS": {"units": 33, "bidirectional": False},
}
INPUT_A = (3, 18, 8, 3)
CONFIG_B = {
    "n_classes": 4, "filters": 8, "first_kernel_size": 3, "first_pool_size": [5, 1],
    "BLOCK0": "mother_stage", "BLOCK0_ARGS": dict(CT.MOTHER, depth=1, filters1=6, strides=[1, 2]),
    "BLOCK1": "bidirectional_GRU_block", "BLOCK1_ARGS": {"units": [192, 128, 4]},
    "SED": "simple_dense_stage", "SED_ARGS": {"depth": 1, "units": 8, "dense_activation": "relu", "dropout_rate": 0},
    "DOA": "bidirectional_GRU_stage", "DOA_ARGS": {"depth": 1, "units": 256},
}
INPUT_B = (2, 35, 6, 7)
MODELS = {"A": (CONFIG_A, INPUT_A), "B": (CONFIG_B, INPUT_B)}


@functools.lru_cache(maxsize=None)
def model_reference(name: str, dtype=torch.float64):
    """-> (cfg, shape, w, st, x, ys, yd, ref): one train step and the inference of conv_temporal_oracle"""
    cfg, shape = MODELS[name]
    w, st = CT.random_weights(cfg, shape, seed=11)
    x, ys, yd = CT.synthetic_batch(cfg, shape, seed=23)
    ref = CT.train_step(cfg, shape, w, st, x, ys, yd, doa_loss="MSE", loss_weight=(1.0, 1000.0), lr=1e-3, step=1, dtype=dtype)
    ref["infer"] = CT.inference(cfg, shape, w, st, x, dtype=dtype)
    return cfg, shape, w, st, x, ys, yd, ref
