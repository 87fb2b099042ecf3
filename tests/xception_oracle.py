"""Plain torch-CPU reference of xception_block's kernels, one operation per function (seld_amd/csrc/xception.hip; spec/XCEPTION_BLOCK.md: a unit is
ReLU -> SeparableConv2D(64, 3, use_bias=False) -> BatchNormalization on [B, H, 16, 64] NHWC), with the inputs and the case lists the GPU and CPU tests
share.  Every function takes a torch dtype: float64 is the reference, float32 measures what plain fp32 arithmetic of the same operation loses
(printed beside every kernel error).  Imports without a GPU."""
import numpy as np
import torch
import torch.nn.functional as F

BN_EPS = 1e-3
GATE_MARGIN = 1e-4      # min |pre-activation| the tests establish before a run: no fp32 evaluation of x scale + shift takes a ReLU gate differently
ELEMENTWISE_BAR = 2e-6  # error over the tensor's maximum of an elementwise fp32 output (test_conv_fwd's bar)

# ---- shapes: the smallest that reach each branch of the kernels
DW_FWD_W16 = [(1, 1, 16), (1, 2, 16), (3, 8, 16), (5, 13, 16), (2, 37, 16)]      # (5, 13): 65 workgroups, 65 % 8 = 1: the XCD remap's ragged case
DW_FWD_GENERIC = [(2, 5, 8), (3, 9, 4)]                                          # W != 16: the generic kernel only
UNIT_SHAPES = [(1, 1), (1, 7), (2, 8), (3, 9), (2, 37)]                          # partial tile, exact tiles with an image boundary between, 8 + 1 rows
UNIT_BIG = (260, 25)             # 1040 tiles on xc_unit_fwd's 512 persistent workgroups: three tiles per workgroup, one valid row in every image's last tile
PW_NPIX = [1, 127, 128, 129, 333, 2 * 65536 + 128 + 37]                          # tile edges; the last: > 1024 tiles of 128 pixels on 512 workgroups
PW_NPIX_FUSED_ONLY = PW_NPIX[-1]
BN_NPIX = [1, 15, 16, 17, 333, 8192 + 53]                                        # 16 pixels per workgroup pass; the last: > 512 workgroups' worth, the strided pass
DW_BWD_BIG = (9, 59)             # 531 rows (> 512 for dw3x3_bwd_w), 133 fused slabs (a third, partial group of 64; a ragged last fold group)


def T(a, dtype=torch.float64):
    return torch.as_tensor(np.asarray(a)).to(dtype)


# ---- inputs
def unit_inputs(B, H, W=16, seed=0):
    """x ~ N(0,1), k = 0.3 N, wpw = N / 8, scale ~ 1 +- 0.5 with negative channels, shift = 0.3 N  (all float32)"""
    rng = np.random.default_rng(1000 * B + 10 * H + W + seed)
    x = rng.standard_normal((B, H, W, 64)).astype(np.float32)
    k = (rng.standard_normal((3, 3, 64)) * 0.3).astype(np.float32)
    wpw = (rng.standard_normal((64, 64)) / 8).astype(np.float32)
    scale = (1.0 + 0.5 * rng.standard_normal(64)).astype(np.float32)
    scale[[3, 17, 40]] = [-0.7, -1.2, -0.4]
    shift = (0.3 * rng.standard_normal(64)).astype(np.float32)
    return x, k, wpw, np.concatenate([scale, shift])


def pre_activation(x, aff):
    """float64 x scale + shift (aff = [scale 64 | shift 64]) or x: what the unit's ReLU sees"""
    x = np.asarray(x, np.float64)
    return x if aff is None else x * np.asarray(aff[:64], np.float64) + np.asarray(aff[64:], np.float64)


def gate_margin(x, aff):
    return float(np.abs(pre_activation(x, aff)).min())


def apply_gate_margin(x, aff, margin=GATE_MARGIN):
    """Move every element whose pre-activation lies within `margin` of zero away from it (by 0.01 / scale, on the side it is on), so that
    min |x scale + shift| >= margin in float64.  Returns (float32 x, number of elements moved)."""
    x = np.array(x, np.float32)
    sc = np.ones(64) if aff is None else np.asarray(aff[:64], np.float64)
    moved = 0
    for _ in range(4):
        pre = pre_activation(x, aff)
        bad = np.abs(pre) < margin
        if not bad.any():
            break
        moved += int(bad.sum())
        step = np.where(pre >= 0, 0.01, -0.01) / sc
        x = np.where(bad, (x.astype(np.float64) + step).astype(np.float32), x)
    return x, moved


# ---- the unit's forward
def depthwise_forward(x, kdw, aff=None, dtype=torch.float64):
    """relu(x scale + shift) or relu(x), then DepthwiseConv2D(3, 'same', use_bias=False); kdw [3][3][C]"""
    a = T(x, dtype)
    C = a.shape[-1]
    if aff is not None:
        a = a * T(aff[:C], dtype) + T(aff[C:], dtype)
    kern = T(kdw, dtype).permute(2, 0, 1).reshape(C, 1, 3, 3)
    return F.conv2d(torch.relu(a).permute(0, 3, 1, 2), kern, padding=1, groups=C).permute(0, 2, 3, 1)


def unit_forward(x, kdw, wpw, aff=None, dtype=torch.float64):
    """-> dwo, z = dwo wpw, sum z, sum z^2 (per channel, over the pixels)"""
    dwo = depthwise_forward(x, kdw, aff, dtype)
    z = dwo @ T(wpw, dtype)
    return dwo, z, z.sum((0, 1, 2)), (z * z).sum((0, 1, 2))


# ---- BatchNormalization (training mode, biased variance, eps 1e-3)
def bn_batch(z, dtype=torch.float64):
    """z [..., C] -> mean, invstd of the batch"""
    z = T(z, dtype).reshape(-1, np.shape(z)[-1])
    mean = z.mean(0)
    var = ((z - mean) ** 2).mean(0)
    return mean, torch.rsqrt(var + BN_EPS)


def bn_train(z, gamma, beta):
    mean = z.reshape(-1, z.shape[-1]).mean(0)
    var = ((z - mean) ** 2).reshape(-1, z.shape[-1]).mean(0)
    return (z - mean) * torch.rsqrt(var + BN_EPS) * gamma + beta


def bn_stats(z, dtype=torch.float64):
    z = T(z, dtype).reshape(-1, np.shape(z)[-1])
    return z.sum(0), (z * z).sum(0)


def bn_apply(z, scale, shift, res=None, dtype=torch.float64):
    out = T(z, dtype) * T(scale, dtype) + T(shift, dtype)
    return out if res is None else out + T(res, dtype)


def bn_backward(z, dy, gamma, dtype=torch.float64):
    """autograd through y = BatchNorm(training)(z): -> dz, dgamma, dbeta, and the batch's mean, invstd, c1 = sum dy / n, c2 = sum dy xhat / n"""
    zt = T(z, dtype).reshape(-1, np.shape(z)[-1]).clone().requires_grad_(True)
    g = T(gamma, dtype).clone().requires_grad_(True)
    b = torch.zeros_like(g).requires_grad_(True)
    d = T(dy, dtype).reshape(zt.shape)
    dz, dg, db = torch.autograd.grad(bn_train(zt, g, b), (zt, g, b), d)
    mean, invstd = bn_batch(zt.detach(), dtype)
    n = zt.shape[0]
    return {"dz": dz, "dgamma": dg, "dbeta": db, "mean": mean, "invstd": invstd, "c1": db / n, "c2": dg / n}


def pw_backward(dwo, wpw, gamma, gy, dtype=torch.float64):
    """autograd through y = BatchNorm(training)(dwo wpw), given gy = dL/dy: -> z, f1 = dL/d dwo, dw = dL/d wpw, and the BatchNorm quantities the
    kernel is handed (mean, invstd, c1, c2 of the same batch)"""
    a = T(dwo, dtype).reshape(-1, 64).clone().requires_grad_(True)
    w = T(wpw, dtype).clone().requires_grad_(True)
    g = T(gamma, dtype)
    z = a @ w
    d = T(gy, dtype).reshape(z.shape)
    f1, dw = torch.autograd.grad(bn_train(z, g, torch.zeros_like(g)), (a, w), d)
    zd = z.detach()
    mean, invstd = bn_batch(zd, dtype)
    n = zd.shape[0]
    xhat = (zd - mean) * invstd
    return {"z": zd, "f1": f1, "dw": dw, "mean": mean, "invstd": invstd, "c1": d.sum(0) / n, "c2": (d * xhat).sum(0) / n}


def module_forward(h, units):
    """one middle-flow module in float64: three units (kdw, wpw, gamma, beta) chained through BatchNormalization, plus the residual"""
    y = T(h)
    for kdw, wpw, gamma, beta in units:
        _, z, _, _ = unit_forward(y, kdw, wpw)
        y = bn_train(z, T(gamma), T(beta))
    return T(h) + y


# ---- error measures
def rel_err_abs_sum(got, ref, terms):
    """error of a per-channel sum of signed terms over max_c sum |term|: what fp32 accumulation is bounded by (the sum's own maximum may be cancelled)"""
    den = float(np.abs(np.asarray(terms, np.float64)).reshape(-1, np.shape(terms)[-1]).sum(0).max())
    return float(np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)).max() / (den if den > 0 else 1.0))
