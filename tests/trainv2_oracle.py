"""fp64 restatement (torch, autograd for the gradients) of the per-step work of the reference's trainv2.py that is not the model:
the weighted losses (trainv2.py:38-44, losses.py:16-34), the L2 kernel regulariser (utils.py:343-350, trainv2.py:46-48), AGC
(utils.py:67-96), AdaBelief (utils.py:157-182) and SWA (swa.py:25-32).  The model itself is oracle.seldnet_oracle's.

The reference evaluates its graph in float32, so its clip bounds are the float32 constants float32(1e-7) and float32(1) - float32(1e-7)
(= 1 - 2^-23, not 1 - 1e-7): the restatement takes those values, everything else is fp64 arithmetic on the float32 inputs."""
import math

import numpy as np
import torch

EPS32 = float(np.float32(1e-7))
HI32 = float(np.float32(1.0) - np.float32(1e-7))
TRAIN_SAMPLES = (58193, 32794, 29801, 21478, 14822, 9174, 66527, 6740, 9342, 6498, 22218, 49758)      # trainv2.py:25-29


def t64(a):
    return torch.as_tensor(np.asarray(a, np.float64))


def smooth(y_sed, ls):
    """trainv2.py:38-39"""
    return y_sed * (1 - ls) + 0.5 * ls if ls > 0 else y_sed


def binary_crossentropy(t, p):
    """tf.keras.backend.binary_crossentropy (trainv2.py:293), elementwise: clip to [eps, 1 - eps], eps inside both logarithms."""
    p = torch.clamp(p, EPS32, HI32)
    return -(t * torch.log(p + EPS32) + (1 - t) * torch.log(1 - p + EPS32))


def focal_loss(t, p, alpha=0.25, gamma=2.0):
    """losses.focal_loss (losses.py:29-34): a scalar."""
    p = torch.clamp(p, EPS32, HI32)
    f = -t * alpha * torch.pow(1 - p, gamma) * torch.log(p) - (1 - t) * alpha * torch.pow(p, gamma) * torch.log(1 - p)
    return f.mean()


def mmse_with_cls_weights(y_true, y_pred, w=None):
    """losses.MMSE_with_cls_weights (losses.py:16-26)."""
    sh = y_true.shape
    sed = torch.round((y_true.reshape(*sh[:-1], 3, -1) ** 2).sum(dim=-2))
    if w is not None:
        sed = sed * w
    sed = torch.cat([sed] * 3, dim=-1)
    return (((y_true - y_pred) ** 2) * sed).sum() / sed.sum()


def losses_v2(sed, doa, y_sed, y_doa, w, sed_loss="BCE", loss_weights=(1.0, 1000.0), ls=0.0, alpha=0.25, gamma=2.0):
    """trainv2.py:38-44 -> (objective without the regulariser, sloss, dloss); all scalars."""
    t = smooth(y_sed, ls)
    if sed_loss == "BCE":
        sloss = (binary_crossentropy(t, sed) * w).mean()
    else:
        sloss = (focal_loss(t, sed, alpha, gamma) * w).mean()       # a scalar times the weight row, then the mean
    dloss = mmse_with_cls_weights(y_doa, doa, w)
    return sloss * loss_weights[0] + dloss * loss_weights[1], sloss, dloss


def losses_v2_pre_grads(sed, doa, y_sed, y_doa, w, **kw):
    """The same from the float32 head OUTPUTS, with the objective's gradients w.r.t. the heads' pre-activations: d / d sed * sed (1 - sed)
    (sigmoid), d / d doa * (1 - doa^2) (tanh)."""
    p = t64(sed).requires_grad_(True)
    d = t64(doa).requires_grad_(True)
    obj, sl, dl = losses_v2(p, d, t64(y_sed), t64(y_doa), t64(w), **kw)
    gp, gd = torch.autograd.grad(obj, (p, d))
    with torch.no_grad():
        return {"sloss": sl.detach().numpy(), "dloss": dl.detach().numpy(), "dsed_pre": (gp * p * (1 - p)).numpy(),
                "ddoa_pre": (gd * (1 - d * d)).numpy()}


# ------------------------------------------------------------------------------------------------ regulariser, AGC, AdaBelief
def unitwise_norm(x):
    """utils.py:67-83"""
    if x.dim() <= 1:
        return (x ** 2).sum() ** 0.5
    if x.dim() in (2, 3):
        return (x ** 2).sum(dim=0, keepdim=True) ** 0.5
    if x.dim() == 4:
        return (x ** 2).sum(dim=(0, 1, 2), keepdim=True) ** 0.5
    raise ValueError("unsupported rank")


def agc(p, g, clip_factor=0.01, eps=1e-3):
    """utils.adaptive_clip_grad for one variable (utils.py:89-95) -> (new gradient, grad_norm / max_norm per unit)."""
    max_norm = torch.clamp(unitwise_norm(p), min=eps) * clip_factor
    gn = unitwise_norm(g)
    clipped = g * (max_norm / torch.clamp(gn, min=1e-6))
    return torch.where(gn < max_norm, g, clipped), (gn / max_norm).reshape(-1)


def adabelief(theta, g, m, v, step, lr=1e-3, b1=0.9, b2=0.999, eps=1e-7):
    """utils.AdaBelief._resource_apply_dense, amsgrad=False (utils.py:162-182) with _prepare_local's lr (utils.py:132-138); step is 1-based."""
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * (g - m) * (g - m)
    lr_t = lr * math.sqrt(1 - b2 ** step) / (1 - b1 ** step)
    return theta - lr_t * m / (torch.sqrt(v) + eps), m, v


def reg_agc_adabelief(theta, g, m, v, shapes, reg, step, lr=1e-3, b1=0.9, b2=0.999, eps=1e-7, l2=0.0, clip_factor=0.01):
    """One v2 optimizer stage over flat buffers holding variables of the Keras `shapes` back to back: the regulariser's gradient 2 l2 w on
    the flagged variables (d / dw of l2 sum(w^2), trainv2.py:46-48), AGC on the sum (clip_factor <= 0: none), AdaBelief.
    -> dict(theta, m, v, g = the gradient the optimizer consumed, ratio = grad_norm / max_norm of every unit)."""
    theta, g, m, v = (t64(a) for a in (theta, g, m, v))
    gs, ratios, off = [], [], 0
    for shape, flag in zip(shapes, reg):
        n = int(np.prod(shape))
        p_, g_ = theta[off:off + n].reshape(shape), g[off:off + n].reshape(shape)
        if flag:
            g_ = g_ + 2 * l2 * p_
        if clip_factor > 0:
            g_, r = agc(p_, g_, clip_factor)
            ratios.append(r)
        gs.append(g_.reshape(-1))
        off += n
    assert off == theta.numel()
    gp = torch.cat(gs)
    th, m1, v1 = adabelief(theta, gp, m, v, step, lr, b1, b2, eps)
    return {"theta": th.numpy(), "m": m1.numpy(), "v": v1.numpy(), "g": gp.numpy(),
            "ratio": torch.cat(ratios).numpy() if ratios else np.zeros(0)}


def swa_update(swa, w, cnt):
    """swa.py:29-31 on float32 arrays, as numpy evaluates it (each operation rounded to float32)."""
    swa, w = np.asarray(swa, np.float32), np.asarray(w, np.float32)
    return ((swa * np.float32(cnt) + w) / np.float32(cnt + 1)).astype(np.float32)


def swa_fires(epoch, start_epoch, swa_freq=2):
    """swa.py:8, 14-19: start_epoch is stored minus one."""
    e = epoch - (start_epoch - 1)
    return e == 0 or (e > 0 and e % swa_freq == 0)


def is_regularized(name):
    """DESIGN.md "The trainv2 recipe": the kernel of a Conv2D, Conv1D or Dense layer, by seld_variable_info's names."""
    return name.endswith(".kernel") and not name.startswith("gru")


def train_step_v2(spec, flat_w, flat_state, x, y_sed, y_doa, w_cls, *, sed_loss="BCE", loss_weights=(1.0, 1000.0), ls=0.0):
    """trainv2.trainstep's forward + losses + tape.gradient (trainv2.py:33-50) WITHOUT the regulariser term, whose gradient
    reg_agc_adabelief adds: outputs, losses, the flat gradient and the new BatchNorm state."""
    from oracle import seldnet_oracle as O
    tr, nt = O.variable_specs(spec)
    fw = t64(flat_w).clone().requires_grad_(True)
    sed, doa, new_st = O.forward(spec, O.unflatten(fw, tr), O.unflatten(t64(flat_state), nt), t64(x), training=True)
    obj, sl, dl = losses_v2(sed, doa, t64(y_sed), t64(y_doa), t64(w_cls), sed_loss=sed_loss, loss_weights=loss_weights, ls=ls)
    (g,) = torch.autograd.grad(obj, fw)
    return {"sed": sed.detach().numpy(), "doa": doa.detach().numpy(), "sloss": sl.detach().numpy(), "dloss": dl.detach().numpy(),
            "grad": g.numpy(), "new_state": torch.cat([new_st[name].reshape(-1) for name, _ in nt]).detach().numpy()}
