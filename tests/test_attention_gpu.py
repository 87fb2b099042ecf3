"""The attention operators (seld_attn_*, seld_ln_*: seld_amd/csrc/attention.hip) and the transformer encoder block / stage composed from them
(seld_amd/modules.py; reference modules.py:106-126, 379-407) on the device against the fp64 restatement tests/transformer_oracle.py, at
the project's bar (helpers.check: max|d| / max|ref| <= 1e-4), and models.seldnet with SECOND = transformer_encoder_stage in a test step and
a train step.

One gradient is zero by mathematics: the key bias shifts every logit of a query row by the same amount, which softmax does not see (at
S = 1 the same holds for the query and key inputs).  The rule of tests/test_modules_gpu.py:143-145 applies as written: where the
reference gradient's maximum is below 1e-9 of the largest gradient, |got| <= 1e-3 * the largest gradient is asserted instead."""
import copy
import ctypes as C
import math

import numpy as np
import pytest
import torch

import transformer_oracle as T
from helpers import check, dev, ptr

pytestmark = pytest.mark.gpu


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _check_or_zero(name, got, ref, biggest):
    if np.abs(ref).max() < 1e-9 * biggest:
        assert np.abs(got).max() <= 1e-3 * biggest, name
    else:
        check(name, got, ref)


# ---------------------------------------------------------------- attention
def _attention_run(lib, q, k, v, do, B, S, H, d, scale, fused, save=True):
    """q, k, v, do: numpy [B, S, H, d] -> (o, lse, dq, dk, dv) as numpy; fused: the operands are column slices of one [B*S, 3*H*d + 8] buffer
    (and the gradients of another), else contiguous"""
    HD = H * d
    R = B * S
    if fused:
        ld = 3 * HD + 8
        buf = torch.full((R, ld), float("nan"), device="cuda")
        gbuf = torch.full((R, ld), float("nan"), device="cuda")
        views = [buf[:, i * HD:(i + 1) * HD] for i in range(3)]
        gviews = [gbuf[:, i * HD:(i + 1) * HD] for i in range(3)]
        for t, a in zip(views, (q, k, v)):
            t.copy_(dev(a.reshape(R, HD)))
    else:
        ld = HD
        views = [dev(a.reshape(R, HD)) for a in (q, k, v)]
        gviews = [torch.full((R, HD), float("nan"), device="cuda") for _ in range(3)]
    o = torch.full((R, HD), float("nan"), device="cuda")
    lse = torch.full((B, H, S), float("nan"), device="cuda") if save else None
    rc = lib.seld_attn_fwd(ptr(views[0]), ptr(views[1]), ptr(views[2]), ld, ld, ld, ptr(o), ptr(lse), B, S, H, d, scale, _stream())
    assert rc == 0
    if not save:
        torch.cuda.synchronize()
        return o.cpu().numpy()
    n = lib.seld_attn_bwd_scratch(B, S, H, d)
    scratch = torch.full((n,), float("nan"), device="cuda")
    god = dev(do.reshape(R, HD))
    rc = lib.seld_attn_bwd(ptr(views[0]), ptr(views[1]), ptr(views[2]), ld, ld, ld, ptr(o), ptr(god), ptr(lse), ptr(gviews[0]), ptr(gviews[1]),
                           ptr(gviews[2]), ld, ld, ld, ptr(scratch), B, S, H, d, scale, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    if fused:      # the columns between and behind the slices were not touched
        assert bool(torch.isnan(gbuf[:, 3 * HD:]).all()) and bool(torch.isnan(buf[:, 3 * HD:]).all())
    return [o.cpu().numpy(), lse.cpu().numpy()] + [g.contiguous().cpu().numpy() for g in gviews]


@pytest.mark.parametrize("B,S,H,d", [(2, 600, 4, 32), (3, 61, 4, 24), (2, 130, 4, 48), (1, 1, 2, 8)])
def test_attention_forward_and_backward(seld_lib, B, S, H, d):
    rng = np.random.default_rng(S)
    q, k, v, do = (rng.standard_normal((B, S, H, d)) for _ in range(4))
    scale = 1.0 / math.sqrt(d)
    tq, tk, tv = (torch.tensor(a, requires_grad=True) for a in (q, k, v))
    o_ref, lse_ref = T.attention(tq, tk, tv, scale)
    gq, gk, gv = torch.autograd.grad((o_ref * torch.tensor(do)).sum(), (tq, tk, tv))
    R, HD = B * S, H * d
    biggest = max(float(g.abs().max()) for g in (gq, gk, gv))
    runs = {}
    for fused in (False, True):
        got = runs[fused] = _attention_run(seld_lib, q, k, v, do, B, S, H, d, scale, fused)
        tag = f"attention {'fused' if fused else 'contiguous'} "
        check(tag + "O", got[0], o_ref.detach().numpy().reshape(R, HD))
        check(tag + "lse", got[1], lse_ref.detach().numpy())
        for name, g, r in zip(("dQ", "dK", "dV"), got[2:], (gq, gk, gv)):
            _check_or_zero(tag + name, g, r.numpy().reshape(R, HD), biggest)      # S = 1: dQ = dK = 0 exactly
    # the strides change addresses only; a second run gives the same bits; so does the forward without the log-sum-exp
    for a, b in zip(runs[False], runs[True]):
        assert np.array_equal(a, b)
    again = _attention_run(seld_lib, q, k, v, do, B, S, H, d, scale, False)
    for a, b in zip(runs[False], again):
        assert np.array_equal(a, b)
    assert np.array_equal(_attention_run(seld_lib, q, k, v, do, B, S, H, d, scale, False, save=False), runs[False][0])


# ---------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("rows,Cc", [(7, 8), (1200, 128), (60, 4378), (3, 1)])
def test_layer_norm_forward_and_backward(seld_lib, rows, Cc, residual):
    lib = seld_lib
    rng = np.random.default_rng(rows + Cc)
    x, r, dy = rng.standard_normal((rows, Cc)) * 2 + 0.5, rng.standard_normal((rows, Cc)), rng.standard_normal((rows, Cc))
    gamma, beta = 1 + 0.3 * rng.standard_normal(Cc), 0.2 * rng.standard_normal(Cc)
    tx, tr_, tg, tb = (torch.tensor(a, requires_grad=True) for a in (x, r, gamma, beta))
    y_ref = T.layer_norm(tx + tr_ if residual else tx, tg, tb)
    gx, gg, gb = torch.autograd.grad((y_ref * torch.tensor(dy)).sum(), (tx, tg, tb))
    dx_, dr_, dg_, db_, ddy = dev(x), dev(r) if residual else None, dev(gamma), dev(beta), dev(dy)
    y, xhat, rstd, dz = (torch.full(s, float("nan"), device="cuda") for s in ((rows, Cc), (rows, Cc), (rows,), (rows, Cc)))
    dgamma, dbeta = torch.full((Cc,), float("nan"), device="cuda"), torch.full((Cc,), float("nan"), device="cuda")
    scratch = torch.full((lib.seld_ln_scratch(rows, Cc),), float("nan"), device="cuda")
    assert lib.seld_ln_fwd(ptr(dx_), ptr(dr_), ptr(dg_), ptr(db_), T.LN_EPS, ptr(y), ptr(xhat), ptr(rstd), rows, Cc, _stream()) == 0
    assert lib.seld_ln_bwd(ptr(ddy), ptr(xhat), ptr(rstd), ptr(dg_), ptr(dz), ptr(dgamma), ptr(dbeta), ptr(scratch), rows, Cc, _stream()) == 0
    y2 = torch.full((rows, Cc), float("nan"), device="cuda")
    assert lib.seld_ln_fwd(ptr(dx_), ptr(dr_), ptr(dg_), ptr(db_), T.LN_EPS, ptr(y2), None, None, rows, Cc, _stream()) == 0
    torch.cuda.synchronize()
    check("LayerNorm y", y.cpu().numpy(), y_ref.detach().numpy())
    assert torch.equal(y, y2)      # the inference form (nothing saved) gives the same bits
    if Cc == 1:
        # one feature: xhat = 0, y = beta, and the input's gradient is 0 exactly
        assert float(dz.abs().max()) <= 1e-3 * float(np.abs(dy).max()) and float(gx.abs().max()) < 1e-12
        assert float(dgamma.abs().max()) <= 1e-3 * float(gb.abs().max())
    else:
        check("LayerNorm dz", dz.cpu().numpy(), gx.numpy())
        check("LayerNorm dgamma", dgamma.cpu().numpy(), gg.numpy())
    check("LayerNorm dbeta", dbeta.cpu().numpy(), gb.numpy())


# ---------------------------------------------------------------- the block and the stage
def _stage_case(B, S, D, H, dk, ffm, k, depth, seed, activation="relu"):
    from oracle import seldnet_oracle as O
    from seld_amd import modules
    cfg = {"depth": depth, "n_head": H, "key_dim": dk, "ff_multiplier": ffm, "kernel_size": k, "dropout_rate": 0, "activation": activation}
    stage = (modules.transformer_encoder_stage if depth > 1 else modules.transformer_encoder_block)(cfg)((B, S, D))
    rt = stage.blocks[0].rt
    rt.finalize()
    specs = T.stage_specs(D, cfg, depth)
    assert [(n, s) for n, _, s in rt.variables] == specs and rt.n_state == 0
    w = T.random_block_weights(specs, seed)
    rng = np.random.default_rng(seed)
    x, dy = rng.standard_normal((B, S, D)), rng.standard_normal((B, S, D))
    rt.params[:rt.n_params].copy_(torch.as_tensor(w))
    xd = dev(x.reshape(B * S, D))
    out = stage.forward(xd, B, True).cpu().numpy().copy()
    out_eval = stage.forward(xd, B, False).cpu().numpy().copy()
    stage.forward(xd, B, True)
    dx = stage.backward(dev(dy.reshape(B * S, D)), B).cpu().numpy().copy()
    grads = rt.grads[:rt.n_params].cpu().numpy().copy()
    fw = torch.tensor(w, dtype=torch.float64, requires_grad=True)
    xt = torch.tensor(x, requires_grad=True)
    yt = T.stage_forward(xt, O.unflatten(fw, specs), cfg, depth)
    gw, gx = torch.autograd.grad((yt * torch.tensor(dy)).sum(), (fw, xt))
    check("transformer forward", out, yt.detach().numpy().reshape(B * S, D))
    assert np.array_equal(out, out_eval)      # no dropout, no batch statistics: training and inference agree bit for bit
    check("transformer input gradient", dx, gx.numpy().reshape(B * S, D))
    off, biggest = 0, float(gw.abs().max())
    for n, s in specs:
        kk = int(np.prod(s))
        _check_or_zero(f"transformer grad {n}", grads[off:off + kk], gw.numpy()[off:off + kk], biggest)
        off += kk


@pytest.mark.parametrize("B,S,D,H,dk,ffm,k", [(2, 600, 128, 4, 32, 2, 1), (3, 61, 96, 4, 24, 4, 3)])
def test_transformer_encoder_block(B, S, D, H, dk, ffm, k):
    _stage_case(B, S, D, H, dk, ffm, k, depth=1, seed=S)


def test_transformer_encoder_stage_of_two_blocks():
    _stage_case(3, 61, 96, 4, 24, 4, 3, depth=2, seed=4, activation="swish")


# ---------------------------------------------------------------- the model
@pytest.mark.parametrize("doa_loss", ["MSE", "MMSE"])
def test_train_step_with_a_transformer_encoder_stage(seldnet_config, doa_loss):
    """models.seldnet with FIRST = mother_stage (the arguments of test_train_step_with_a_mother_stage_first_block) and SECOND =
    transformer_encoder_stage: one test step and one train step against the fp64 oracle — variable list, outputs, both losses, every
    gradient, BatchNorm state, post-Adam weights — then a batch of 2 on the model built for 3"""
    from oracle import seldnet_oracle as O
    from seld_amd import losses, models, train
    from test_modules_gpu import STAGE_FIRST
    cfg = copy.deepcopy(seldnet_config)
    cfg["FIRST"], cfg["FIRST_ARGS"] = "mother_stage", copy.deepcopy(STAGE_FIRST)
    cfg["SECOND"] = "transformer_encoder_stage"
    cfg["SECOND_ARGS"] = {"depth": 2, "n_head": 4, "key_dim": 24, "ff_multiplier": 2, "kernel_size": 1, "dropout_rate": 0}
    B, T_ = 3, 100
    in_shape = (B, T_, 64, 7)
    tr, nt = T.variable_specs(cfg, in_shape)
    w, st = T.random_weights(cfg, in_shape, seed=11)
    x, ys, yd = O.synthetic_batch(B, T_, seed=23)
    model = models.seldnet(in_shape, cfg)
    assert type(model).__name__ == "ComposedSeldNet"
    assert [(n, s) for n, _, s in model.variables] == tr and [(n, s) for n, _, s in model.state_variables] == nt
    assert sum(n.startswith("tf") for n, _ in tr) == 32 and not any(n.startswith("gru") for n, _ in tr)
    model.set_weights(w, st)
    fw = torch.tensor(w, dtype=torch.float64)
    sed_t, doa_t, _ = T.forward(cfg, O.unflatten(fw, tr), O.unflatten(torch.tensor(st, dtype=torch.float64), nt), torch.tensor(x, dtype=torch.float64), False)
    y_t, sl_t, dl_t = train.teststep(model, x, (ys, yd), losses.BinaryCrossentropy(), losses.get_doa_loss(doa_loss))
    check("transformer model teststep sed", y_t[0].cpu().numpy(), sed_t.numpy())
    check("transformer model teststep doa", y_t[1].cpu().numpy(), doa_t.numpy())
    ref = T.train_step(cfg, in_shape, w, st, x, ys, yd, doa_loss=doa_loss, loss_weight=(1.0, 1000.0), lr=1e-3, step=1)
    y_p, sl, dl = train.trainstep(model, x, (ys, yd), losses.BinaryCrossentropy(), losses.get_doa_loss(doa_loss), (1.0, 1000.0), train.Adam(1e-3))
    check("transformer model trainstep sed", y_p[0].cpu().numpy(), ref["sed"])
    check("transformer model trainstep doa", y_p[1].cpu().numpy(), ref["doa"])
    check("transformer model sloss", sl.cpu().numpy(), ref["sloss"])
    check("transformer model dloss", dl.cpu().numpy(), ref["dloss"])
    g = model.get_grads()
    for n, off, sh in model.variables:
        k = int(np.prod(sh))
        r = ref["grad"][off:off + k]
        if np.abs(r).max() < 1e-9 * np.abs(ref["grad"]).max():      # conv biases in front of training-mode BatchNormalization; the key biases
            assert np.abs(g[off:off + k]).max() <= 1e-3 * np.abs(ref["grad"]).max(), n
            continue
        check(f"transformer model grad {n}", g[off:off + k], r)
    w1, st1 = model.get_weights()
    check("transformer model BN state", st1, ref["new_state"])
    big = np.abs(ref["grad"]) > 1e-3 * np.abs(ref["grad"]).max()
    assert np.abs(w1 - ref["new_w"])[big].max() <= 2e-3 * 1e-3 + 1e-7       # Adam's first step moves a weight by lr g / (|g| + eps)
    # a batch of 2 on the model built for 3
    y2 = model(x[:2], training=False)
    sed2, doa2, _ = T.forward(cfg, O.unflatten(torch.tensor(w1, dtype=torch.float64), tr), O.unflatten(torch.tensor(st1, dtype=torch.float64), nt),
                              torch.tensor(x[:2], dtype=torch.float64), False)
    assert tuple(y2[0].shape) == (2, T_ // 5, 12)
    check("transformer model batch of 2 sed", y2[0].cpu().numpy(), sed2.numpy())
    check("transformer model batch of 2 doa", y2[1].cpu().numpy(), doa2.numpy())
    y3, _, _ = train.trainstep(model, x[:2], (ys[:2], yd[:2]), losses.BinaryCrossentropy(), losses.get_doa_loss(doa_loss), (1.0, 1000.0), train.Adam(1e-3))
    assert tuple(y3[1].shape) == (2, T_ // 5, 36) and bool(torch.isfinite(y3[0]).all()) and np.isfinite(model.get_grads()).all()
