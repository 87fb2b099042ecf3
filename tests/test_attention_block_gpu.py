"""Relative-position attention (seld_relattn_*, seld_glu_*: seld_amd/csrc/relattn.hip) and the attention block / stage composed from it
(seld_amd/modules.py; reference modules.py:155-180, 511-635, layers.py:332-392) on the device against the fp64 restatement
tests/attention_block_oracle.py, at the project's bar (helpers.check: max|d| / max|ref| <= 1e-4 per tensor; tests/test_attention_block_cpu.py
holds that a plain fp32 evaluation of every case here stays within 5e-5), and models.seldnet with SECOND = attention_stage in a train step.

Gradients that are zero by mathematics follow the rule of tests/test_attention_gpu.py (_check_or_zero): the key bias, and at S = 1 whatever
only moves the single logit."""
import copy
import functools

import numpy as np
import pytest
import torch

import attention_block_oracle as A
from helpers import check, dev, ptr, rel_err
from test_attention_gpu import _Window, _check_or_zero, _stream

pytestmark = pytest.mark.gpu

OUTS = ("O", "lse", "dQu", "dQv", "dK", "dV", "dP")


@functools.lru_cache(maxsize=None)
def _reference(B, S, H, d):
    ins = A.relattn_inputs(B, S, H, d)
    return ins, A.relattn_reference(*ins)


def _run(lib, ins, B, S, H, d, fused=False, save=True, rows_for=None):
    """seld_relattn_fwd (+ _bwd when save) -> dict of numpy.  fused: Q, K, V are column slices of one [B*S, 3*H*d + 8] buffer and dQu, dQv, dK
    of another; rows_for: the batch the buffers are sized for (>= B).  Every output sits in a NaN-filled allocation whose surroundings must keep
    the sentinel's bits."""
    q, k, v, P, u, vb, do, scale = ins
    HD, R, Ra = H * d, B * S, (rows_for or B) * S
    band = 64 * HD + 1
    pad = lambda a: np.concatenate([np.asarray(a).reshape(R, HD), np.zeros((Ra - R, HD))]) if Ra > R else np.asarray(a).reshape(R, HD)
    if fused:
        ld = 3 * HD + 8
        src = torch.full((Ra, ld), float("nan"), device="cuda")
        for i, a in enumerate((q, k, v)):
            src[:, i * HD:(i + 1) * HD] = dev(pad(a))
        pq, pk, pv = (ptr(src[:, i * HD:]) for i in range(3))
        dst = torch.full((Ra, ld), float("nan"), device="cuda")
        gq, gv_, gk = (dst[:, i * HD:(i + 1) * HD] for i in range(3))
        pgq, pgv, pgk = (ptr(dst[:, i * HD:]) for i in range(3))
        ldg = ld
    else:
        ld = ldg = HD
        wq, wk, wv = (_Window(Ra, HD, None, None, band, band, pad(a)) for a in (q, k, v))
        pq, pk, pv = wq.ptr(), wk.ptr(), wv.ptr()
        wgq, wgv, wgk = (_Window(Ra, HD, None, None, band, band) for _ in range(3))
        pgq, pgv, pgk = wgq.ptr(), wgv.ptr(), wgk.ptr()
    wp = _Window(S, HD, None, None, band, band, P)
    wu, wvb = _Window(1, HD, None, None, band, band, u), _Window(1, HD, None, None, band, band, vb)
    wo, wl = _Window(Ra, HD, None, None, band, band), _Window((rows_for or B) * H, S, None, None, band, band)
    rc = lib.seld_relattn_fwd(pq, pk, pv, ld, ld, ld, wp.ptr(), HD, wu.ptr(), wvb.ptr(), wo.ptr(), wl.ptr() if save else None, B, S, H, d, scale,
                              _stream())
    assert rc == 0
    torch.cuda.synchronize()
    wo.assert_band("O")
    out = {"O": wo.numpy()[:R].reshape(B, S, H, d)}
    if not save:
        return out
    wl.assert_band("lse")
    out["lse"] = wl.numpy()[:B * H].reshape(B, H, S)
    n = lib.seld_relattn_bwd_scratch(B, S, H, d)
    assert n == B * H * S * (1 + 2 * d)
    ws = _Window(1, n, None, None, band, band)
    wdo = _Window(Ra, HD, None, None, band, band, pad(do))
    wdv, wdp = _Window(Ra, HD, None, None, band, band), _Window(S, HD, None, None, band, band)
    for w in (wp, wu, wvb, wdo, wo, wl):
        w.snapshot()
    rc = lib.seld_relattn_bwd(pq, pk, pv, ld, ld, ld, wp.ptr(), HD, wu.ptr(), wvb.ptr(), wo.ptr(), wdo.ptr(), wl.ptr(), pgq, pgv, pgk, wdv.ptr(),
                              wdp.ptr(), ldg, ldg, ldg, HD, HD, ws.ptr(), B, S, H, d, scale, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    for name, w in zip(("P", "u", "vb", "dO", "O", "lse"), (wp, wu, wvb, wdo, wo, wl)):
        w.assert_unchanged(name)
    for name, w in (("dV", wdv), ("dP", wdp), ("scratch", ws)):
        w.assert_band(name)
    if fused:
        assert bool(torch.isnan(dst[:, 3 * HD:]).all()) and bool(torch.isnan(dst[R:]).all())
        got = [t[:R].contiguous().cpu().numpy() for t in (gq, gv_, gk)]
    else:
        for name, w in (("dQu", wgq), ("dQv", wgv), ("dK", wgk)):
            w.assert_band(name)
        got = [w.numpy()[:R] for w in (wgq, wgv, wgk)]
    for name, a in zip(("dQu", "dQv", "dK"), got):
        out[name] = a.reshape(B, S, H, d)
    out["dV"] = wdv.numpy()[:R].reshape(B, S, H, d)
    if Ra > R:
        assert bool(torch.isnan(wdv.view[R:]).all()) and bool(torch.isnan(wo.view[R:]).all())      # rows of the larger batch stay untouched
    out["dP"] = wdp.numpy().reshape(S, H, d)
    return out


@pytest.mark.parametrize("B,S,H,d", A.RELATTN_CASES)
def test_relattn_forward_and_backward_against_the_oracle(seld_lib, B, S, H, d):
    ins, ref = _reference(B, S, H, d)
    got = _run(seld_lib, ins, B, S, H, d)
    biggest = max(float(np.abs(ref[n]).max()) for n in OUTS[2:])
    for n in OUTS[:2]:
        check(f"relattn {(B, S, H, d)} {n}", got[n], ref[n])
    for n in OUTS[2:]:
        _check_or_zero(f"relattn {(B, S, H, d)} {n}", got[n], ref[n], biggest)


@pytest.mark.parametrize("B,S,H,d", [(2, 65, 3, 8), (3, 100, 4, 16)])
def test_relattn_strided_slices_null_lse_and_a_second_run(seld_lib, B, S, H, d):
    """Q / K / V as column slices of one fused [B*S, 3 H d + 8] buffer change addresses only; lse = NULL leaves O's bits; a second backward gives
    the same bits (no atomics, fixed orders)"""
    ins, ref = _reference(B, S, H, d)
    a = _run(seld_lib, ins, B, S, H, d)
    b = _run(seld_lib, ins, B, S, H, d, fused=True)
    c = _run(seld_lib, ins, B, S, H, d)
    for n in OUTS:
        assert np.array_equal(a[n], b[n]), f"{n}: strided"
        assert np.array_equal(a[n], c[n]), f"{n}: second run"
    assert np.array_equal(_run(seld_lib, ins, B, S, H, d, save=False)["O"], a["O"])


def test_relattn_smaller_batch_on_buffers_sized_for_a_larger_one(seld_lib):
    B, S, H, d = 2, 65, 3, 8
    ins, ref = _reference(B, S, H, d)
    got = _run(seld_lib, ins, B, S, H, d, rows_for=3)
    for n in OUTS:
        check(f"relattn b < B {n}", got[n], ref[n])


@pytest.mark.parametrize("B,S,H,d", [(2, 65, 3, 8), (2, 130, 2, 64)])
def test_relattn_without_positions_is_plain_attention(seld_lib, B, S, H, d):
    """u = vb = 0 and P = 0: the logits are seld_attn_fwd's (which scales the query instead of the sum) to 1e-6"""
    q, k, v, P, u, vb, do, scale = A.relattn_inputs(B, S, H, d)
    got = _run(seld_lib, (q, k, v, 0 * P, 0 * u, 0 * vb, do, scale), B, S, H, d, save=False)["O"]
    HD, R = H * d, B * S
    o = torch.full((R, HD), float("nan"), device="cuda")
    dq, dk, dv = (dev(a.reshape(R, HD)) for a in (q, k, v))
    assert seld_lib.seld_attn_fwd(ptr(dq), ptr(dk), ptr(dv), HD, HD, HD, ptr(o), None, B, S, H, d, scale, _stream()) == 0
    torch.cuda.synchronize()
    assert rel_err(got.reshape(R, HD), o.cpu().numpy()) <= 1e-6


@pytest.mark.parametrize("rows,Cc,span", [(1, 1, 0.0), (130, 5, 0.0), (64, 64, 0.0), (130, 5, 40.0)])
def test_glu_forward_and_backward(seld_lib, rows, Cc, span):
    """span 40: gates of +-40, where sigmoid'(40) = 4.2e-18 is lost by s (1 - s) on a rounded s"""
    rng = np.random.default_rng([rows, Cc])
    u, dy = A.f32(rng.standard_normal((rows, 2 * Cc))), A.f32(rng.standard_normal((rows, Cc)))
    if span:
        u[:, Cc:] = np.where(rng.random((rows, Cc)) < 0.5, span, -span)
    tu = torch.tensor(u, requires_grad=True)
    y = A.CF.glu(tu)
    (gu,) = torch.autograd.grad((y * torch.tensor(dy)).sum(), tu)
    for ld in (2 * Cc, 2 * Cc + 3):
        wu, wy = _Window(rows, 2 * Cc, ld, None, 65, 65, u), _Window(rows, Cc, None, None, 65, 65)
        wdy, wdu = _Window(rows, Cc, None, None, 65, 65, dy), _Window(rows, 2 * Cc, ld, None, 65, 65)
        assert seld_lib.seld_glu_fwd(wu.ptr(), ld, wy.ptr(), rows, Cc, _stream()) == 0
        assert seld_lib.seld_glu_bwd(wu.ptr(), ld, wdy.ptr(), wdu.ptr(), ld, rows, Cc, _stream()) == 0
        torch.cuda.synchronize()
        wy.assert_band("y"), wdu.assert_band("du")
        check(f"glu {(rows, Cc, span)} y", wy.numpy(), y.detach().numpy())
        check(f"glu {(rows, Cc, span)} du", wdu.numpy(), gu.numpy())
        if span:
            g2, r2 = wdu.numpy()[:, Cc:], gu.numpy()[:, Cc:]
            assert 0 < np.abs(r2).max() < 1e-15 and np.abs(g2 - r2).max() <= 1e-4 * np.abs(r2).max()


# ---------------------------------------------------------------- the block and the stage
@pytest.mark.parametrize("name", sorted(A.STAGE_CASES))
def test_attention_block_and_stage(name):
    """forward in training and in inference (inference follows the moving statistics the training step left), the input's and every variable's
    gradient"""
    from seld_amd import modules
    B, S, D, depth, cfg = A.STAGE_CASES[name]
    ref = A.stage_reference(B, S, D, depth, cfg, seed=3)
    tr, nt = ref["specs"]
    stage = (modules.attention_stage if "depth" in cfg else modules.attention_block)(cfg)((B, S, D))
    rt = stage.blocks[0].rt
    rt.finalize()
    assert [(n, s) for n, _, s in rt.variables] == tr and [(n, s) for n, _, s in rt.state_variables] == nt
    rt.params[:rt.n_params].copy_(torch.as_tensor(ref["w"]))
    if rt.n_state:
        rt.state[:rt.n_state].copy_(torch.as_tensor(ref["st"]))
    xd = dev(ref["x"].reshape(B * S, D))
    out = stage.forward(xd, B, True).cpu().numpy().copy()
    state = rt.state[:rt.n_state].cpu().numpy().copy()
    out_eval = stage.forward(xd, B, False).cpu().numpy().copy()
    if rt.n_state:
        rt.state[:rt.n_state].copy_(torch.as_tensor(ref["st"]))
    stage.forward(xd, B, True)
    dx = stage.backward(dev(ref["dy"].reshape(B * S, D)), B).cpu().numpy().copy()
    grads = rt.grads[:rt.n_params].cpu().numpy().copy()
    tag = f"attention_block {name}"
    check(f"{tag} forward (training)", out, ref["out_train"].reshape(B * S, D))
    check(f"{tag} forward (inference)", out_eval, ref["out_eval"].reshape(B * S, D))
    if rt.n_state:
        check(f"{tag} moving statistics", state, ref["new_state"])
        assert np.abs(out - out_eval).max() > 1e-3 * np.abs(out).max()
    check(f"{tag} input gradient", dx, ref["dx"].reshape(B * S, D))
    off, biggest = 0, float(np.abs(ref["grad"]).max())
    for n, s in tr:
        kk = int(np.prod(s))
        _check_or_zero(f"{tag} grad {n}", grads[off:off + kk], ref["grad"][off:off + kk], biggest)
        off += kk


# ---------------------------------------------------------------- the model
def test_train_step_with_an_attention_stage(seldnet_config):
    """models.seldnet with a small mother_block FIRST (8 + 8 filters: d_model 240) and SECOND = attention_stage (relative positions): variable
    list, outputs, both losses, every gradient, BatchNorm state and the post-Adam weights of one train step against the fp64 oracle"""
    from oracle import seldnet_oracle as O
    from seld_amd import losses, models, train
    from test_modules_gpu import STAGE_FIRST
    cfg = A.model_case(seldnet_config, STAGE_FIRST)
    B, T_ = A.MODEL_INPUT[:2]
    in_shape = A.MODEL_INPUT
    tr, nt = A.variable_specs(cfg, in_shape)
    w, st = A.random_weights(cfg, in_shape, seed=11)
    x, ys, yd = O.synthetic_batch(B, T_, seed=23)
    model = models.seldnet(in_shape, cfg)
    assert type(model).__name__ == "ComposedSeldNet"
    assert [(n, s) for n, _, s in model.variables] == tr and [(n, s) for n, _, s in model.state_variables] == nt
    assert any(n == "at1.mha.pos_bias_v" for n, _ in tr) and not any(n.startswith("gru") for n, _ in tr)
    model.set_weights(w, st)
    ref = A.train_step(cfg, in_shape, w, st, x, ys, yd, doa_loss="MSE", loss_weight=(1.0, 1000.0), lr=1e-3, step=1)
    y_p, sl, dl = train.trainstep(model, x, (ys, yd), losses.BinaryCrossentropy(), losses.get_doa_loss("MSE"), (1.0, 1000.0), train.Adam(1e-3))
    check("attention model trainstep sed", y_p[0].cpu().numpy(), ref["sed"])
    check("attention model trainstep doa", y_p[1].cpu().numpy(), ref["doa"])
    check("attention model sloss", sl.cpu().numpy(), ref["sloss"])
    check("attention model dloss", dl.cpu().numpy(), ref["dloss"])
    g = model.get_grads()
    biggest = np.abs(ref["grad"]).max()
    for n, off, sh in model.variables:
        k = int(np.prod(sh))
        _check_or_zero(f"attention model grad {n}", g[off:off + k], ref["grad"][off:off + k], biggest)
    w1, st1 = model.get_weights()
    check("attention model BN state", st1, ref["new_state"])
    big = np.abs(ref["grad"]) > 1e-3 * biggest
    assert np.abs(w1 - w)[big].min() > 0
    assert np.abs(w1 - ref["new_w"])[big].max() <= 2e-3 * 1e-3 + 1e-7       # Adam's first step moves a weight by lr g / (|g| + eps)
