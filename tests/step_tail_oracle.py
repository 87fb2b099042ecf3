"""float64 restatements of seld_amd/csrc/loss_adam.hip's kernels, one function per kernel family, with the case tables that
tests/test_step_tail_gpu.py runs and tests/test_step_tail_cpu.py checks without a device.  Every reference takes the float32 values a kernel
reads as exact numbers; the losses' gradients are those w.r.t. the heads' PRE-activations, formed analytically from the stored outputs
(p (1 - p), 1 - d^2) as the kernels form them.  oracle/seldnet_oracle.py states the operations; this module only adds what the kernels'
arguments need (strides, one variable of a flat buffer, the coupling's chain rule, the time layout) and the float32-constant BinaryCrossentropy.

Each *_f32 function is the same formula evaluated in float32 on the CPU, in the kernel's order of operations where the order matters: the CPU
tests hold it within half of each bar, which shows the bar leaves room for a correct float32 kernel and none for much else."""
import functools

import numpy as np
import torch

from oracle import seldnet_oracle as O

F64 = torch.float64
LOSS_MODES = {"MSE": 0, "MMSE": 1, "MAE": 2, "MSLE": 3}
LOSS_WEIGHT = (1.0, 1000.0)
# (B, S, nc): one row; one partial workgroup; 64 rows with nc % 4 == 2; 65 rows (a workgroup of one live and 63 dead rows) with nc % 4 == 1;
# 4 097 rows = 65 workgroups: losses_finalize_kernel's second lap, reduce_rows_kernel's fifth, 17 blocks of mmse_mask_rows_kernel
LOSS_SHAPES = [(1, 1, 12), (1, 63, 12), (4, 16, 14), (5, 13, 5), (17, 241, 12)]
STRIDED_SHAPES = [(5, 13, 5), (17, 241, 12)]
TOL = {"sloss": 1e-4, "dloss": 1e-4, "ddoa_pre": 1e-4, "dsed_pre": 2e-4}      # tests/helpers.check bars of test_kernels_gpu.py::test_losses

# the reference program runs in float32: K.epsilon() and 1 - K.epsilon() as float32 numbers (0.99999988 = 1 - 2^-23, not 0.9999999)
BCE_LO = float(np.float32(1e-7))
BCE_HI = float(np.float32(1) - np.float32(1e-7))


def t64(a):
    return torch.as_tensor(np.asarray(a), dtype=F64)


# ------------------------------------------------------------------------------------------------ losses
def bce_f32_bounds(y, p):
    """tf.keras.losses.BinaryCrossentropy() with the clip bounds and the epsilon inside the logarithms as the float32 constants a float32
    TensorFlow program holds, promoted to float64.  Equal to seldnet_oracle.bce wherever no element is clipped from above (the CPU tests pin
    that); on an element at p = 0.99999994 or 1 with y = 0 the two differ by 6e-3 of the element's value."""
    pc = torch.clamp(p, BCE_LO, BCE_HI)
    return (-(y * torch.log(pc + BCE_LO) + (1 - y) * torch.log(1 - pc + BCE_LO))).mean()


@functools.lru_cache(maxsize=None)
def _labels(B, S, nc):
    _, ys, yd = O.synthetic_batch(B, S * 5, n_classes=nc, seed=11)
    return ys, yd


def loss_inputs(B, S, nc, seed=8, ties=True):
    """Head outputs and labels as float32: labels from synthetic_batch (active and silent classes), logits drawn as in
    test_kernels_gpu.py::test_losses (3 N(0, 1) with four saturated ones in the first row; N(0, 1) for the DOA head), outputs = float32 of the
    float64 sigmoid / tanh.  ties: a few DOA outputs are set to their labels, zero labels included (MAE's subgradient at 0)."""
    rng = np.random.default_rng(seed + 1000 * B + S)
    ys, yd = _labels(B, S, nc)
    sp = rng.standard_normal((B, S, nc)) * 3
    sp[0, 0, :4] = [40, -40, 20, -20]
    if B * S > 64:      # the last row is confidently wrong (p = sigmoid(-+8)): the last workgroup's partial is >= 1e-3 of sloss even as one row of 4 097
        sp[-1, -1] = 8 - 16 * ys[-1, -1]
    dp = rng.standard_normal((B, S, 3 * nc))
    sed = torch.sigmoid(t64(sp)).numpy().astype(np.float32)
    doa = torch.tanh(t64(dp)).numpy().astype(np.float32)
    if ties:
        flat, yflat = doa.reshape(-1), yd.reshape(-1)
        idx = np.unique(np.concatenate([np.arange(0, flat.size, 7), np.flatnonzero(yflat)[::3]]))
        flat[idx] = yflat[idx]
    return sed, doa, ys.astype(np.float32), yd.astype(np.float32)


def tie_mask(doa, yd):
    return np.asarray(doa) == np.asarray(yd)


def losses_ref(sed, doa, ys, yd, mode, lw=LOSS_WEIGHT, sed_grad_scale=1.0, mmse_den=0.0, dtype=F64):
    """sloss [1], dloss ([rows] or [1]), dsed_pre [B,S,nc], ddoa_pre [B,S,3nc] of train.py:24-31's objective, from the stored head outputs.
    mmse_den > 0 replaces MMSE's denominator (seld_loss_cfg.mmse_den).  dtype float32 gives the *_f32 evaluation."""
    p = torch.as_tensor(np.asarray(sed)).to(dtype).requires_grad_(True)
    q = torch.as_tensor(np.asarray(doa)).to(dtype).requires_grad_(True)
    y1, y3 = torch.as_tensor(np.asarray(ys)).to(dtype), torch.as_tensor(np.asarray(yd)).to(dtype)
    _, _, dl = O.losses_and_objective(p, q, y1, y3, mode, lw)
    if mode == "MMSE" and mmse_den > 0:
        nc = y1.shape[-1]
        m = torch.round((y3.reshape(*y3.shape[:-1], 3, nc) ** 2).sum(dim=-2))
        dl = (((y3 - q) ** 2) * torch.cat([m] * 3, dim=-1)).sum() / mmse_den
    sl = bce_f32_bounds(y1, p)
    obj = (sl * lw[0] * sed_grad_scale + dl * lw[1]).sum()
    gp, gq = torch.autograd.grad(obj, (p, q))
    pd, qd = p.detach(), q.detach()
    return {"sloss": sl.detach().reshape(1).numpy(), "dloss": dl.detach().reshape(-1).numpy(), "dsed_pre": (gp * pd * (1 - pd)).numpy(),
            "ddoa_pre": (gq * (1 - qd * qd)).numpy()}


def bce_boundary_case():
    """One [1, 2, 12] row set: every p of the clip's neighbourhood against y = 0, 1 and 0.3.  Returns sed, y_sed and the mask of elements whose
    gradient the clip blocks (p outside [float32(1e-7), 0.99999988]): exactly 0 there."""
    lo, hi = np.float32(1e-7), np.float32(1) - np.float32(1e-7)
    ps = np.array([0.0, 5e-8, lo, np.nextafter(lo, np.float32(1)), 0.5, hi, np.nextafter(hi, np.float32(2)), 1.0], np.float32)
    assert ps[6] == np.float32(0.99999994) and ps[5] == np.float32(0.99999988)
    sed = np.repeat(ps, 3).reshape(1, 2, 12)
    ys = np.tile(np.array([0.0, 1.0, 0.3], np.float32), 8).reshape(1, 2, 12)
    blocked = (sed < lo) | (sed > hi)
    return sed, ys, blocked


# ------------------------------------------------------------------------------------------------ Adam
ADAM_NS = [1, 255, 256, 257]
ADAM_STEPS = [1, 1000, 100000]


def adam_case(n, step):
    """theta, g, m, v (float32) with a slice where g = m = v = 0 (theta keeps its bits there), and the slice"""
    rng = np.random.default_rng(n * 7 + step)
    th, g, m, v = (rng.standard_normal(n).astype(np.float32) for _ in range(4))
    v = np.abs(v)
    z = slice(n // 2, n // 2 + n // 8)
    g[z] = m[z] = v[z] = 0
    return th, g, m, v, z


ADAM_HYPER = {"lr": 1e-3, "b1": 0.9, "b2": 0.999, "eps": 1e-7}


def adam_ref(th, g, m, v, step, dtype=F64):
    """adam_update with the hyper-parameters as the float32 numbers the entry point receives (as a float32 Keras optimizer holds them): they are
    inputs like theta and g.  float32(0.9) is 2.6e-8 below 0.9; where m' = b1 m + (1 - b1) g cancels to a hundredth of its terms (the one-element
    case at step 1 000) a reference at 0.9 in double is 2.7e-6 of the result away from any float32 Adam."""
    conv = lambda a: torch.as_tensor(a).to(dtype)
    return [t.numpy() for t in O.adam_update(conv(th), conv(g), conv(m), conv(v), step=step, **{k: float(np.float32(x)) for k, x in ADAM_HYPER.items()})]


# ------------------------------------------------------------------------------------------------ AGC
AGC_SHAPES = [(384,), (1,), (128, 384), (1, 257), (1, 128, 12), (3, 128, 36), (3, 3, 7, 64), (3, 3, 64, 64), (3, 3, 256, 32)]
AGC_OFF = 37          # floats in front of the variable inside the flat buffers
AGC_TOL = 1e-5        # test_model_gpu.py::test_train_step_agc's bar; units of at most 576 elements
AGC_TOL_MAX = 1e-4    # ceiling of the measured bar of the 2 304-element units


def agc_rows_cols(shape):
    """the [rows][cols] view of a Keras variable with one clip unit per column (utils.unitwise_norm)"""
    if len(shape) == 1:
        return shape[0], 1
    if len(shape) == 2:
        return shape[0], shape[1]
    if len(shape) == 3:
        return shape[0], shape[1] * shape[2]
    return shape[0] * shape[1] * shape[2], shape[3]


def agc_case(shape):
    """theta, g (float32, Keras shape) and the intended decision per unit.  Units alternate between clipped (gn = 1.3 .. 4 max_norm) and kept
    (gn = 0.2 .. 0.8 max_norm), so half of every variable's units take each branch (rank 1 has one unit: the two rank-1 cases take one branch
    each).  Variables of at least 8 units carry three forced ones: unit 1 has an all-zero gradient, units 2 and 3 all-zero parameters (the
    ceiling is max(0, 1e-3) * 0.01 = 1e-5), one above it and one below."""
    rows, cols = agc_rows_cols(shape)
    ci = AGC_SHAPES.index(tuple(shape))
    rng = np.random.default_rng(100 + ci)
    th = (rng.standard_normal((rows, cols)) * 0.05).astype(np.float32)
    g = rng.standard_normal((rows, cols))
    clip = (np.arange(cols) + ci) % 2 == 0
    if cols >= 8:
        th[:, 2:4] = 0
    ratio = np.where(clip, rng.uniform(1.3, 4.0, cols), rng.uniform(0.2, 0.8, cols))
    pn = np.sqrt((th.astype(np.float64) ** 2).sum(axis=0))
    max_norm = np.maximum(pn, 1e-3) * 0.01
    g = (g * (ratio * max_norm / np.sqrt((g ** 2).sum(axis=0)))).astype(np.float32)
    if cols >= 8:
        g[:, 1] = 0
        clip[1] = False
    return th.reshape(shape), g.reshape(shape), clip


def agc_ratio(th, g):
    """gn / max_norm per unit in float64"""
    rows, cols = agc_rows_cols(th.shape)
    t, gg = th.reshape(rows, cols).astype(np.float64), g.reshape(rows, cols).astype(np.float64)
    return np.sqrt((gg ** 2).sum(axis=0)) / (np.maximum(np.sqrt((t ** 2).sum(axis=0)), 1e-3) * 0.01)


def agc_ref(th, g):
    return O.adaptive_clip_grad([t64(th)], [t64(g)])[0].numpy()


def agc_f32(th, g):
    """agc_kernel in float32 on the CPU: both sums run over a unit's elements in row order, one add per element"""
    rows, cols = agc_rows_cols(th.shape)
    t, gg = th.reshape(rows, cols), g.reshape(rows, cols).copy()
    pn, gn = np.zeros(cols, np.float32), np.zeros(cols, np.float32)
    for r in range(rows):
        pn += t[r] * t[r]
        gn += gg[r] * gg[r]
    pn, gn = np.sqrt(pn), np.sqrt(gn)
    max_norm = np.maximum(pn, np.float32(1e-3)) * np.float32(0.01)
    sc = np.where(gn < max_norm, np.float32(1), max_norm / np.maximum(gn, np.float32(1e-6))).astype(np.float32)
    return (gg * sc).reshape(th.shape)


def unit_err(got, ref):
    """worst over the units of max |got - ref| / max |ref| within the unit (1 for an all-zero unit): no unit hides behind a larger one"""
    rows, cols = agc_rows_cols(ref.shape)
    a, b = np.asarray(got, np.float64).reshape(rows, cols), np.asarray(ref, np.float64).reshape(rows, cols)
    den = np.abs(b).max(axis=0)
    return float((np.abs(a - b).max(axis=0) / np.where(den > 0, den, 1.0)).max())


def agc_tol(shape):
    """1e-5 for units of at most 576 elements.  Above (the 2 304-element units of [3, 3, 256, 32]) the serial float32 sums have no ceiling that
    tight: four times the error of the float32 CPU evaluation in the kernel's order, at most 1e-4."""
    rows, _ = agc_rows_cols(shape)
    if rows <= 576:
        return AGC_TOL
    th, g, _ = agc_case(shape)
    return min(4 * unit_err(agc_f32(th, g), agc_ref(th, g)), AGC_TOL_MAX)


# ------------------------------------------------------------------------------------------------ heads' activation backward
ACT_NS = [4, 1020, 1024, 1028]


def act_case(n, act):
    """a stored output y = act(.) with the activation's end values planted (sigmoid 0 and 1, tanh -1 and 1, relu 0), and dy.  Element 1 is
    act(0.3) with dy = 1.5 in every case: the bar is relative to the largest |result|, and 1 - y^2 in float32 carries 2^-24 of absolute error
    wherever y is near 1, so a four-element case of saturated outputs alone would measure that against a result of 1e-3."""
    rng = np.random.default_rng(n + act)
    z = rng.standard_normal(n) * 2
    z[1] = 0.3
    z = t64(z)
    y = {1: torch.sigmoid(z), 2: torch.tanh(z), 3: torch.relu(z)}[act].numpy().astype(np.float32)
    ends = {1: [0.0, 1.0], 2: [-1.0, 1.0], 3: [0.0, 0.0]}[act]
    y[0], y[n - 1] = ends
    if n >= 1020:
        y[1016], y[1019] = ends[::-1]      # the last float4 of the first 255: the block edge of 1 024 and 1 028
    dy = rng.standard_normal(n).astype(np.float32)
    dy[1] = 1.5
    return y, dy


def act_bwd_ref(y, dy, act, dtype=np.float64):
    y, dy = y.astype(dtype), dy.astype(dtype)
    return dy * (y * (1 - y) if act == 1 else 1 - y * y if act == 2 else (y > 0))


# ------------------------------------------------------------------------------------------------ seldnet_v1 coupling
V1_SHAPES = [(1, 12), (65, 5), (300, 14)]


def v1_inputs(rows, nc):
    """sed = sigmoid(b), doa1 = tanh(a) as float32, and labels ([1, rows, .] blocks of synthetic_batch)"""
    rng = np.random.default_rng(rows + nc)
    sed = torch.sigmoid(t64(rng.standard_normal((1, rows, nc)) * 2)).numpy().astype(np.float32)
    doa1 = torch.tanh(t64(rng.standard_normal((1, rows, 3 * nc)))).numpy().astype(np.float32)
    ys, yd = _labels(1, rows, nc)
    return sed, doa1, ys.astype(np.float32), yd.astype(np.float32)


def v1_couple(sed, doa1):
    return torch.tanh(doa1 * torch.cat([sed] * 3, dim=-1))


def v1_fwd_ref(sed, doa1, dtype=F64):
    return v1_couple(torch.as_tensor(sed).to(dtype), torch.as_tensor(doa1).to(dtype)).numpy()


def v1_bwd_ref(sed, doa1, ys, yd, mode, lw=LOSS_WEIGHT, dtype=F64, closed_form=False):
    """Gradients of the objective on (sed, tanh(doa1 * tile(sed, 3))) w.r.t. the two heads' pre-activations b and a (sed = sigmoid(b),
    doa1 = tanh(a)), from the stored outputs.  closed_form: the kernels' two-stage route (the losses' gradient w.r.t. the coupled output's
    pre-activation u = doa1 sed, then d a = du sed (1 - doa1^2), d b += sum_k du_k doa1_k sed (1 - sed)) instead of autograd through it."""
    s = torch.as_tensor(sed).to(dtype).requires_grad_(True)
    d1 = torch.as_tensor(doa1).to(dtype).requires_grad_(True)
    y1, y3 = torch.as_tensor(ys).to(dtype), torch.as_tensor(yd).to(dtype)
    nc = s.shape[-1]
    if closed_form:
        r = losses_ref(sed, v1_couple(s.detach(), d1.detach()).numpy(), ys, yd, mode, lw, dtype=dtype)
        du, sd, dd = torch.as_tensor(r["ddoa_pre"]), s.detach(), d1.detach()
        s3 = torch.cat([sd] * 3, dim=-1)
        acc = (du * dd).reshape(*du.shape[:-1], 3, nc).sum(dim=-2)
        return {"dsed_pre": (torch.as_tensor(r["dsed_pre"]) + acc * sd * (1 - sd)).numpy(), "ddoa_pre": (du * s3 * (1 - dd * dd)).numpy()}
    _, _, dl = O.losses_and_objective(s, v1_couple(s, d1), y1, y3, mode, lw)
    obj = (bce_f32_bounds(y1, s) * lw[0] + dl * lw[1]).sum()
    gs, gd = torch.autograd.grad(obj, (s, d1))
    sd, dd = s.detach(), d1.detach()
    return {"dsed_pre": (gs * sd * (1 - sd)).numpy(), "ddoa_pre": (gd * (1 - dd * dd)).numpy()}


# ------------------------------------------------------------------------------------------------ Conv1D('same') time layout
TIME_KS = [1, 2, 3, 4, 5]
TIME_SHAPES = [(1, 1, 4), (3, 2, 8), (2, 7, 128), (2, 65, 36)]      # S < ks; clip boundaries inside a 256-thread block; several blocks


def time_expand_ref(x, ks):
    """xe[b, t, j C + c] = x[b, t + j - (ks - 1) // 2, c], zero outside the clip (TensorFlow's 'same': the extra pad of an even kernel behind)"""
    B, S, Cc = x.shape
    xe = np.zeros((B, S, ks, Cc), x.dtype)
    for t in range(S):
        for j in range(ks):
            ts = t + j - (ks - 1) // 2
            if 0 <= ts < S:
                xe[:, t, j] = x[:, ts]
    return xe.reshape(B, S, ks * Cc)


def time_fold_ref(dxe, ks, prev=None):
    """the transpose, adds in the array's own precision in tap order on top of `prev` (accumulate) or of zero"""
    B, S, K = dxe.shape
    Cc = K // ks
    d = dxe.reshape(B, S, ks, Cc)
    dx = np.zeros((B, S, Cc), dxe.dtype) if prev is None else prev.copy()
    for j in range(ks):
        for t in range(S):
            tr = t - j + (ks - 1) // 2
            if 0 <= tr < S:
                dx[:, t] = dx[:, t] + d[:, tr, j]
    return dx


def time_case(B, S, Cc, ks):
    rng = np.random.default_rng(B * 1000 + S * 10 + ks)
    return (rng.standard_normal((B, S, Cc)).astype(np.float32), rng.standard_normal((B, S, ks * Cc)).astype(np.float32),
            rng.standard_normal((B, S, Cc)).astype(np.float32))


# ------------------------------------------------------------------------------------------------ dropout, masks
DROP_NS = [4, 1020, 1024, 1028]
DROP_RATES = [0.0, 0.1, 0.5]
DROP_STREAMS = [(16, 0), (97, 12345)]      # (layer, step)
DROP_SEED = 0x1234567887654321


def dropout4_ref(v, rate, seed, layer, step):
    """mask and float32 values of dropout_kernel: kept where philox_uniform >= float32(rate), times the float32 1 / (1 - rate)"""
    r = np.float32(rate)
    keep = O.philox_uniform(v.size, seed, layer, step) >= r
    scale = np.float32(1) / (np.float32(1) - r)
    return keep, np.where(keep, v * scale, np.float32(0)).astype(np.float32)


MASK_SHAPES = [(1, 1, 4), (6, 3, 8), (130, 65, 128)]      # (rows, S, F)


def mask_rows_case(rows, S, F):
    rng = np.random.default_rng(rows + S + F)
    nclip = (rows + S - 1) // S
    mask = np.where(rng.random((nclip, F)) < 0.3, 0.0, 1.0 / 0.7).astype(np.float32)
    return rng.standard_normal((rows, F)).astype(np.float32), mask, rng.standard_normal((rows, F)).astype(np.float32)


def mask_rows_ref(x, mask, S, prev=None, dtype=np.float64):
    out = x.astype(dtype) * np.repeat(mask, S, axis=0)[:x.shape[0]].astype(dtype)
    return out if prev is None else prev.astype(dtype) + out


# ------------------------------------------------------------------------------------------------ which test runs which kernel
# every __global__ of loss_adam.hip -> the GPU tests that run it ("file::test"); tests/test_step_tail_cpu.py checks the kernel list against the
# source and that every named test exists
COVERAGE = {
    "reduce_rows_kernel": ["test_step_tail_gpu.py::test_losses_against_fp64"],
    "mmse_mask_rows_kernel": ["test_step_tail_gpu.py::test_losses_against_fp64"],
    "den_store_kernel": ["test_step_tail_gpu.py::test_losses_against_fp64"],
    "losses_kernel": ["test_step_tail_gpu.py::test_losses_against_fp64", "test_step_tail_gpu.py::test_losses_strided_outputs",
                      "test_step_tail_gpu.py::test_bce_clip_boundary"],
    "losses_finalize_kernel": ["test_step_tail_gpu.py::test_losses_against_fp64", "test_step_tail_gpu.py::test_losses_deferred_finalize"],
    "adam_kernel": ["test_step_tail_gpu.py::test_adam_block_edges_and_late_steps", "test_kernels_gpu.py::test_adam"],
    "agc_kernel": ["test_step_tail_gpu.py::test_agc_one_variable"],
    "act_bwd_kernel": ["test_step_tail_gpu.py::test_act_bwd"],
    "v1_couple_fwd_kernel": ["test_step_tail_gpu.py::test_v1_couple_fwd"],
    "v1_couple_bwd_kernel": ["test_step_tail_gpu.py::test_v1_couple_bwd_behind_the_losses"],
    "time_expand_kernel": ["test_step_tail_gpu.py::test_time_expand_and_fold"],
    "time_fold_kernel": ["test_step_tail_gpu.py::test_time_expand_and_fold"],
    "dropout_kernel": ["test_step_tail_gpu.py::test_dropout4"],
    "mask_rows_kernel": ["test_step_tail_gpu.py::test_mask_rows"],
    "fill_kernel": ["test_step_tail_gpu.py::test_fill_sets_the_given_mmse_denominator"],
}
