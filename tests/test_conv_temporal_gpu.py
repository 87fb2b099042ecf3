"""models.conv_temporal on the device: the stem operators (seld_stem_conv_fwd / _wgrad, seld_pool2d_fwd / _bwd: seld_amd/csrc/stem.hip) one by
one, and the composed model (modules.ConvTemporalNet) against the fp64 restatement tests/conv_temporal_oracle.py at the project's bar
(helpers.check: max|d| / max|ref| <= 1e-4).  The pooling kernels move values and do no arithmetic: they are compared bit for bit.

Every operand of an operator call sits inside a NaN-filled allocation (test_attention_gpu._Window) with a band in front and behind: after
the call every float outside the windows still holds the sentinel's bits.  Gradients that are zero by mathematics (a convolution's bias in
front of training-mode BatchNormalization, the attention's key bias) follow the rule of tests/test_attention_gpu.py (_check_or_zero)."""
import copy
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import conv_temporal_oracle as CT
from conftest import ROOT
from helpers import check, dev
from oracle import modules_oracle as M
from oracle import seldnet_oracle as O
from test_attention_gpu import _Window, _check_or_zero, _stream

pytestmark = pytest.mark.gpu

SS5_PATH = os.path.join(ROOT, "tests", "golden", "SS5.json")
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)

# ---------------------------------------------------------------- the stem convolution
# (B, H, W, Cin, k, F): the SS5 stem on a short clip and on one whole clip (19 row tiles), odd sizes with ten channels (16 slots per pixel) and
# two filter groups, the smallest of everything, one pixel (every tap but the centre lies outside), 16 channels with 33 filters and five
# column tiles
CONV_CASES = [(2, 13, 64, 7, 7, 32), (1, 300, 64, 7, 7, 32), (3, 21, 17, 10, 5, 48), (2, 9, 5, 1, 3, 1), (1, 1, 1, 7, 7, 32), (2, 6, 130, 16, 7, 33)]
# 40 x 4 x 2 = 320 tiles of 8 x 32 pixels: the second stage adds 320 partials; 70 x 1 x 9 = 630 tiles for the 512 first-stage workgroups:
# some walk two tiles (one channel, one filter: the walk is what this case is about)
WGRAD_CASES = CONV_CASES + [(40, 30, 64, 7, 7, 32), (70, 8, 260, 1, 3, 1)]


@functools.lru_cache(maxsize=None)
def _conv_case(B, H, W, Cin, k, F):
    """inputs with a non-zero mean (fp32 values) and the fp64 results -> dict"""
    rng = np.random.default_rng([B, H, W, Cin, k, F])
    f32 = CT.f32
    x = f32(0.5 + rng.standard_normal((B, H, W, Cin)))
    w = f32(0.1 + rng.standard_normal((k, k, Cin, F)) / np.sqrt(k * k * Cin))
    b = f32(0.3 + 0.2 * rng.standard_normal(F))
    dz = f32(0.2 + rng.standard_normal((B, H, W, F)))
    tw, tb = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (w, b))
    z = M.conv2d_same(torch.tensor(x, dtype=torch.float64), tw, tb)
    gw, gb = torch.autograd.grad((z * torch.tensor(dz, dtype=torch.float64)).sum(), (tw, tb))
    return {"x": x, "w": w, "b": b, "dz": dz, "z": z.detach().numpy(), "dw": gw.numpy(), "db": gb.numpy()}


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "x".join(map(str, c)))
def test_stem_conv_forward(seld_lib, case):
    B, H, W, Cin, k, F = case
    ref = _conv_case(*case)
    band = 64 * F + 1
    wx, ww, wb = _Window(B * H * W, Cin, None, None, band, band, ref["x"]), _Window(k * k * Cin, F, None, None, band, band, ref["w"]), \
        _Window(1, F, None, None, band, band, ref["b"])
    outs = []
    for _ in range(2):
        wz = _Window(B * H * W, F, None, None, band, band)
        for t in (wx, ww, wb):
            t.snapshot()
        assert seld_lib.seld_stem_conv_fwd(wx.ptr(), ww.ptr(), wb.ptr(), wz.ptr(), B, H, W, Cin, k, F, _stream()) == 0
        torch.cuda.synchronize()
        for n, t in (("x", wx), ("kernel", ww), ("bias", wb)):
            t.assert_unchanged(n)
        wz.assert_band("z")
        outs.append(wz.numpy())
    check(f"stem conv forward {case}", outs[0].reshape(B, H, W, F), ref["z"])
    assert np.array_equal(bits(outs[0]), bits(outs[1])), "two runs differ"


@pytest.mark.parametrize("case", WGRAD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_stem_conv_weight_gradient(seld_lib, case):
    B, H, W, Cin, k, F = case
    ref = _conv_case(*case)
    band = 64 * F + 1
    n = int(seld_lib.seld_stem_conv_wgrad_scratch(B, H, W, Cin, k, F))
    tiles = B * -(-H // 8) * -(-W // 32)
    assert n == min(tiles, 512) * (k * k * Cin + 1) * F
    wx, wdz = _Window(B * H * W, Cin, None, None, band, band, ref["x"]), _Window(B * H * W, F, None, None, band, band, ref["dz"])
    outs = []
    for _ in range(2):
        wdw, wdb, ws = _Window(k * k * Cin, F, None, None, band, band), _Window(1, F, None, None, band, band), _Window(1, n, None, None, band, band)
        wx.snapshot(), wdz.snapshot()
        assert seld_lib.seld_stem_conv_wgrad(wx.ptr(), wdz.ptr(), wdw.ptr(), wdb.ptr(), ws.ptr(), B, H, W, Cin, k, F, _stream()) == 0
        torch.cuda.synchronize()
        wx.assert_unchanged("x"), wdz.assert_unchanged("dz")
        for nm, t in (("dkernel", wdw), ("dbias", wdb), ("scratch", ws)):
            t.assert_band(nm)
        assert bool(torch.isfinite(ws.view).all()), "a float of the scratch was not written"
        outs.append((wdw.numpy(), wdb.numpy()))
    check(f"stem conv dkernel {case}", outs[0][0].reshape(k, k, Cin, F), ref["dw"])
    check(f"stem conv dbias {case}", outs[0][1].reshape(F), ref["db"])
    assert np.array_equal(bits(outs[0][0]), bits(outs[1][0])) and np.array_equal(bits(outs[0][1]), bits(outs[1][1])), "two runs differ"


# ---------------------------------------------------------------- pooling
POOLS = [(5, 2), (5, 1), (5, 4), (2, 3)]
POOL_HW = [(50, 16), (52, 15), (3, 1)]
POOL_C = [32, 7, 1]


def _pool_run(lib, x, dy, pool, same, with_idx=True, aligned=False):
    """x [B,H,W,C], dy [B,Ho,Wo,C] (None: forward only) -> (y, idx, dx) numpy.  The band in front of every operand is an odd number of floats
    (no pointer is aligned beyond 4 bytes: the scalar kernels) or, `aligned`, a multiple of four (with C % 4 == 0: the float4 kernels)"""
    B, H, W, Cc = x.shape
    Ho, Wo = (-(-H // pool[0]), -(-W // pool[1])) if same else (H // pool[0], W // pool[1])
    band = 64 * Cc + (0 if aligned else 1)
    wx, wy = _Window(B * H * W, Cc, None, None, band, band, x), _Window(B * Ho * Wo, Cc, None, None, band, band)
    idx = torch.full((B * Ho * Wo * Cc + 128,), 255, dtype=torch.uint8, device="cuda")
    iv = idx[64:64 + B * Ho * Wo * Cc]
    wx.snapshot()
    assert lib.seld_pool2d_fwd(wx.ptr(), wy.ptr(), C.c_void_p(iv.data_ptr()) if with_idx else None, B, H, W, Cc, pool[0], pool[1], int(same), _stream()) == 0
    torch.cuda.synchronize()
    wx.assert_unchanged("x"), wy.assert_band("y")
    assert bool((idx[:64] == 255).all()) and bool((idx[64 + iv.numel():] == 255).all())
    if not with_idx:
        assert bool((iv == 255).all())
    dx = None
    if dy is not None:
        wdy, wdx = _Window(B * Ho * Wo, Cc, None, None, band, band, dy), _Window(B * H * W, Cc, None, None, band, band)
        wdy.snapshot()
        saved = idx.clone()
        assert lib.seld_pool2d_bwd(wdy.ptr(), C.c_void_p(iv.data_ptr()), wdx.ptr(), B, H, W, Cc, pool[0], pool[1], int(same), _stream()) == 0
        torch.cuda.synchronize()
        wdy.assert_unchanged("dy"), wdx.assert_band("dx")
        assert torch.equal(idx, saved)
        assert bool(torch.isfinite(wdx.view).all()), "an element of dx was not written"
        dx = wdx.numpy().reshape(B, H, W, Cc)
    return wy.numpy().reshape(B, Ho, Wo, Cc), iv.cpu().numpy().reshape(B, Ho, Wo, Cc), dx


def _first_in_bounds(H, W, pool, same):
    """[H, W] bool: the first in-bounds element, in row-major window order, of every window"""
    ph, pw = pool
    (Ho, hb, _), (Wo, wb, _) = (CT.same_pads(H, ph), CT.same_pads(W, pw)) if same else ((H // ph, 0, 0), (W // pw, 0, 0))
    m = np.zeros((H, W), bool)
    for i in range(Ho):
        for j in range(Wo):
            m[max(i * ph - hb, 0), max(j * pw - wb, 0)] = True
    return m


@pytest.mark.parametrize("hw", POOL_HW, ids=lambda v: "x".join(map(str, v)))
@pytest.mark.parametrize("pool", POOLS, ids=lambda v: "x".join(map(str, v)))
def test_pool2d_forward_and_backward(seld_lib, pool, hw):
    H, W = hw
    B = 2
    for Cc in POOL_C:
        for same in (True, False):
            pad = "same" if same else "valid"
            tag = f"pool {pool} on {hw} x {Cc} {pad}"
            rng = np.random.default_rng([H, W, Cc, pool[0], pool[1], int(same)])
            if not same and (H < pool[0] or W < pool[1]):      # 'valid' leaves nothing (Keras raises): refused before anything is enqueued
                p = dev(np.zeros(64, np.float32))
                pp = C.c_void_p(p.data_ptr())
                assert seld_lib.seld_pool2d_fwd(pp, pp, pp, B, H, W, Cc, pool[0], pool[1], 0, _stream()) == -1, tag
                assert seld_lib.seld_pool2d_bwd(pp, pp, pp, B, H, W, Cc, pool[0], pool[1], 0, _stream()) == -1, tag
                continue
            # distinct values, all negative (a zero padding would win): every window has a unique maximum
            n = B * H * W * Cc
            x = CT.f32((rng.permutation(n).astype(np.float64) - n - 1.0) / 64.0).reshape(B, H, W, Cc)
            xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
            win = CT.pool_windows(xt.detach(), pool, pad)
            top = torch.topk(win, 2, dim=3).values
            assert bool((top[:, :, :, 0] > top[:, :, :, 1]).all()), "the oracle's input has a tie: the comparison could hide one"
            yt = CT.maxpool2d(xt, pool, pad)
            dy = CT.f32(rng.standard_normal(tuple(yt.shape)))
            (gx,) = torch.autograd.grad((yt * torch.tensor(dy, dtype=torch.float64)).sum(), xt)
            y, idx, dx = _pool_run(seld_lib, x, dy, pool, same)
            assert np.array_equal(bits(y), bits(yt.detach().numpy())), tag + ": forward"
            assert np.array_equal(idx, win.argmax(dim=3).numpy()), tag + ": positions"
            assert np.array_equal(bits(dx), bits(gx.numpy())), tag + ": backward"
            for al in ((False, True) if Cc % 4 == 0 else (False,)):
                y0, _, _ = _pool_run(seld_lib, x, None, pool, same, with_idx=False, aligned=al)
                assert np.array_equal(bits(y0), bits(y)), tag + ": idx NULL"
            if Cc % 4 == 0:      # the float4 kernels give the scalar kernels' bits
                ya, ia, dxa = _pool_run(seld_lib, x, dy, pool, same, aligned=True)
                assert np.array_equal(bits(ya), bits(y)) and np.array_equal(ia, idx) and np.array_equal(bits(dxa), bits(dx)), tag + ": float4"
            # all elements equal: the gradient lands on the first in-bounds element of each window
            xe = np.full((B, H, W, Cc), -1.5, np.float32)
            ye, _, dxe = _pool_run(seld_lib, xe, dy, pool, same, aligned=True)
            assert bool((ye == -1.5).all()), tag + ": padding won"
            first = _first_in_bounds(H, W, pool, same)
            want = np.zeros((B, H, W, Cc), np.float32)
            want[:, first] = dy.reshape(B, -1, Cc)
            assert np.array_equal(bits(dxe), bits(want)), tag + ": ties"


# ---------------------------------------------------------------- the model
@functools.lru_cache(maxsize=None)
def _model_ref(name, doa_loss):
    cfg, shape = {"ss5": (CT.SS5_SMALL, CT.SS5_SMALL_INPUT), "chain2": (CT.CHAIN2, CT.CHAIN2_INPUT)}[name]
    w, st = CT.random_weights(cfg, shape, seed=11)
    x, ys, yd = CT.synthetic_batch(cfg, shape, seed=23)
    ref = CT.train_step(cfg, shape, w, st, x, ys, yd, doa_loss=doa_loss, loss_weight=(1.0, 1000.0), lr=1e-3, step=1)
    ref["infer"] = CT.inference(cfg, shape, w, st, x)
    return cfg, shape, w, st, x, ys, yd, ref


def _model_check(name, doa_loss):
    """one test step and one train step against the fp64 oracle — variable list, outputs, both losses, every gradient, BatchNormalization
    state, post-Adam weights — then a smaller batch on the same model: the quantities and bars of
    test_conformer_gpu.test_train_step_with_a_conformer_encoder_stage"""
    from seld_amd import losses, models, train
    cfg, shape, w, st, x, ys, yd, ref = _model_ref(name, doa_loss)
    tr, nt = CT.variable_specs(cfg, shape)
    model = models.conv_temporal(shape, cfg)
    assert type(model).__name__ == "ConvTemporalNet"
    assert [(n, s) for n, _, s in model.variables] == tr and [(n, s) for n, _, s in model.state_variables] == nt
    model.set_weights(w, st)
    tag = f"conv_temporal {name}"
    y_i = model(x, training=False)
    check(f"{tag} inference sed", y_i[0].cpu().numpy(), ref["infer"][0])
    check(f"{tag} inference doa", y_i[1].cpu().numpy(), ref["infer"][1])
    y_t, _, _ = train.teststep(model, x, (ys, yd), losses.BinaryCrossentropy(), losses.get_doa_loss(doa_loss))
    check(f"{tag} teststep sed", y_t[0].cpu().numpy(), ref["infer"][0])
    check(f"{tag} teststep doa", y_t[1].cpu().numpy(), ref["infer"][1])
    st_before = model.get_weights()[1]
    y_f = model(x, training=True)                # a training forward alone: batch statistics, moving statistics updated
    check(f"{tag} training forward sed", y_f[0].cpu().numpy(), ref["sed"])
    check(f"{tag} training forward doa", y_f[1].cpu().numpy(), ref["doa"])
    check(f"{tag} training forward BN state", model.get_weights()[1], ref["new_state"])
    model.set_weights(w, st_before)
    y_p, sl, dl = train.trainstep(model, x, (ys, yd), losses.BinaryCrossentropy(), losses.get_doa_loss(doa_loss), (1.0, 1000.0), train.Adam(1e-3))
    check(f"{tag} trainstep sed", y_p[0].cpu().numpy(), ref["sed"])
    check(f"{tag} trainstep doa", y_p[1].cpu().numpy(), ref["doa"])
    check(f"{tag} sloss", sl.cpu().numpy(), ref["sloss"])
    check(f"{tag} dloss", dl.cpu().numpy(), ref["dloss"])
    g = model.get_grads()
    biggest = np.abs(ref["grad"]).max()
    for n, off, sh in model.variables:
        k = int(np.prod(sh))
        _check_or_zero(f"{tag} grad {n}", g[off:off + k], ref["grad"][off:off + k], biggest)
    w1, st1 = model.get_weights()
    check(f"{tag} BN state", st1, ref["new_state"])
    big = np.abs(ref["grad"]) > 1e-3 * biggest
    assert np.abs(w1 - ref["new_w"])[big].max() <= 2e-3 * 1e-3 + 1e-7       # Adam's first step moves a weight by lr g / (|g| + eps)
    # a batch smaller than the one the model was built for
    nb = shape[0] - 1
    y2 = model(x[:nb], training=False)
    sed2, doa2 = CT.inference(cfg, shape, w1, st1, x[:nb])
    assert tuple(y2[0].shape) == (nb,) + ref["sed"].shape[1:]
    check(f"{tag} batch of {nb} sed", y2[0].cpu().numpy(), sed2)
    check(f"{tag} batch of {nb} doa", y2[1].cpu().numpy(), doa2)
    y3, _, _ = train.trainstep(model, x[:nb], (ys[:nb], yd[:nb]), losses.BinaryCrossentropy(), losses.get_doa_loss(doa_loss), (1.0, 1000.0),
                               train.Adam(1e-3))
    assert tuple(y3[1].shape) == (nb,) + ref["doa"].shape[1:] and bool(torch.isfinite(y3[0]).all()) and np.isfinite(model.get_grads()).all()
    with pytest.raises(ValueError, match="composed models"):      # adaptive gradient clipping stays refused for composed models
        train.trainstep(model, x, (ys, yd), losses.BinaryCrossentropy(), losses.get_doa_loss(doa_loss), (1.0, 1000.0), train.Adam(1e-3), agc=True)


@pytest.mark.parametrize("doa_loss", ["MSE", "MMSE"])
def test_ss5_shaped_model(doa_loss):
    """SS5.json's chain at input (2, 52, 15, 7) (52 frames: 11 pooled frames with 1 row of padding in front and 2 behind; 15 bins: 8 with 1
    behind), every Dropout at 0: mother_stage, simple_dense_stage, conformer stage; a conformer stage (key_dim 48) as the SED head, a
    bidirectional_GRU_stage as the DOA head"""
    _model_check("ss5", doa_loss)


def test_second_chain():
    """mother_block -> RNN_stage (LSTM, concat) -> transformer_encoder_block; SED identity_block, DOA simple_dense_stage; a 3 x 3 stem"""
    _model_check("chain2", "MSE")


@pytest.fixture(scope="module")
def ss5_model(tmp_path_factory):
    """tests/golden/SS5.json verbatim, built for 5 windows of 300 frames through load_conv_temporal_model from a saved .npz -> (model, cfg, w, st)"""
    from seld_amd import evaluator, models
    cfg = json.load(open(SS5_PATH))
    shape = (5, 300, 64, 7)
    w, st = CT.random_weights(cfg, shape, seed=3)
    src = models.conv_temporal((1, 300, 64, 7), cfg)
    src.set_weights(w, st)
    path = str(tmp_path_factory.mktemp("ss5") / "weights.npz")
    src.save_weights(path)
    model = evaluator.load_conv_temporal_model(shape, SS5_PATH, path)
    w1, st1 = model.get_weights()
    assert np.array_equal(bits(w1), bits(w)) and np.array_equal(bits(st1), bits(st))
    return model, cfg, w, st


def test_ss5_json_verbatim(ss5_model):
    """inference of one 300-frame clip (a batch of 1 on the model built for 5) against the oracle; a training forward differs from it: the
    conformer stages name no dropout_rate, so the reference's default 0.1 draws"""
    model, cfg, w, st = ss5_model
    shape = (1, 300, 64, 7)
    x, _, _ = CT.synthetic_batch(cfg, shape, seed=2)
    sed, doa = CT.inference(cfg, shape, w, st, x)
    y = model(x, training=False)
    assert tuple(y[0].shape) == (1, 60, 12) and tuple(y[1].shape) == (1, 60, 36)
    check("SS5.json inference sed", y[0].cpu().numpy(), sed)
    check("SS5.json inference doa", y[1].cpu().numpy(), doa)
    # training: batch statistics AND dropout; with every rate forced to 0 the same forward is deterministic, so the draws are what differs
    y1 = [t.clone() for t in model(x, training=True)]
    y2 = [t.clone() for t in model(x, training=True)]
    assert float((y1[0] - y2[0]).abs().max()) > 1e-4 * float(y1[0].abs().max()), "two training forwards drew the same masks, or none"
    assert float((y1[0] - y[0]).abs().max()) > 1e-4 * float(y[0].abs().max())
    model.set_weights(w, st)


def test_load_conv_temporal_model_and_ensemble_outputs(ss5_model):
    from seld_amd import evaluator
    model, cfg, w, st = ss5_model
    model.set_weights(w, st)
    rng = np.random.default_rng(9)
    clip = CT.f32(0.3 + rng.standard_normal((320, 64, 7)))
    (sed, doa), = evaluator.ensemble_outputs(model, [clip], win_size=300, step_size=5, batch_size=4)      # 5 windows in batches of 4 + 1
    n_win, L = 5, 60
    assert tuple(sed.shape) == (n_win - 1 + L, 12) and tuple(doa.shape) == (n_win - 1 + L, 36)
    wins = np.stack([clip[5 * i:5 * i + 300] for i in range(n_win)])
    ys = [t.cpu().numpy() for t in model(wins, training=False)]
    for got, per_win in ((sed, ys[0]), (doa, ys[1])):
        acc = np.zeros((n_win - 1 + L, per_win.shape[-1]))
        cnt = np.zeros((n_win - 1 + L, 1))
        for i in range(n_win):
            acc[i:i + L] += per_win[i]
            cnt[i:i + L] += 1
        # the same kernels on the same windows, in batches of 4 + 1 here and of 5 above: fp32 rounding apart (a GEMM may tile 4, 1 and 5
        # rows differently), far below the 1e-4 a wrong window or divisor would show at
        check("ensemble_outputs", got.cpu().numpy(), acc / cnt, 1e-5)
    s0, d0 = CT.inference(cfg, (1, 300, 64, 7), w, st, wins[:1])      # and the first window against the oracle
    check("ensemble window 0 sed", ys[0][:1], s0)
    check("ensemble window 0 doa", ys[1][:1], d0)
