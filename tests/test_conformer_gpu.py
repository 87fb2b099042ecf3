"""The conformer operators (seld_dwconv1d_*, seld_pos_add, seld_head_permute: seld_amd/csrc/conformer.hip) and the conformer encoder block /
stage composed from them (seld_amd/modules.py; reference modules.py:129-152, 410-508) on the device against the fp64 restatement
tests/conformer_oracle.py, at the project's bar (helpers.check: max|d| / max|ref| <= 1e-4; tests/test_conformer_cpu.py holds that a plain fp32
evaluation of every case here stays within 5e-5), and models.seldnet with SECOND = conformer_encoder_stage in a test step and a train step.

Gradients that are zero by mathematics follow the rule of tests/test_attention_gpu.py (_check_or_zero): the key bias (softmax does not see
it), the depthwise bias in front of training-mode BatchNormalization, and at S = 1 the query and key kernels and the query bias."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import conformer_oracle as K
from helpers import check, dev, ptr
from test_attention_gpu import _Window, _check_or_zero, _stream

pytestmark = pytest.mark.gpu

KS = [1, 2, 3, 8, 24, 31, 32, 33, 64]
CS = [1, 7, 64, 65, 128, 192]


# ---------------------------------------------------------------- the depthwise kernels alone
def _dw_run(lib, u, w, bias, dy, B, S, Cc, k, glu, ldu=None, lddu=None):
    """seld_dwconv1d_fwd and _bwd with every operand inside a NaN-filled allocation (a band of 64 rows + 1 float in front and behind; row
    strides ldu / lddu, None: contiguous) -> (y, du, dw, dbias) as numpy.  Asserted here: every float outside the windows keeps the sentinel's
    bits, the inputs keep theirs, and every float of seld_dwconv1d_bwd_scratch(...) is written."""
    W, R = (1 + glu) * Cc, B * S
    ldu, lddu = ldu or W, lddu or W
    band = 64 * W + 1
    mk = lambda rows, cols, ld=None, data=None: _Window(rows, cols, ld, None, band, band, data)
    wu, ww, wb, wdy = mk(R, W, ldu, u), mk(k, Cc, None, w), mk(1, Cc, None, bias), mk(R, Cc, None, dy)
    wy, wdu, wdw, wdb = mk(R, Cc), mk(R, W, lddu), mk(k, Cc), mk(1, Cc)
    n = lib.seld_dwconv1d_bwd_scratch(B, S, Cc, k)
    assert (k + 1) * Cc <= n <= 512 * (k + 1) * Cc
    ws = mk(1, n)
    ins = {"u": wu, "w": ww, "bias": wb, "dy": wdy}
    for x in ins.values():
        x.snapshot()
    assert lib.seld_dwconv1d_fwd(wu.ptr(), ldu, ww.ptr(), wb.ptr(), wy.ptr(), B, S, Cc, k, glu, _stream()) == 0
    assert lib.seld_dwconv1d_bwd(wu.ptr(), ldu, ww.ptr(), wdy.ptr(), wdu.ptr(), lddu, wdw.ptr(), wdb.ptr(), ws.ptr(), B, S, Cc, k, glu, _stream()) == 0
    torch.cuda.synchronize()
    for name, x in ins.items():
        x.assert_unchanged(name)
    for name, x in (("y", wy), ("du", wdu), ("dw", wdw), ("dbias", wdb), ("scratch", ws)):
        x.assert_band(name)
    assert bool(torch.isfinite(ws.view).all())
    return [wy.numpy(), wdu.numpy(), wdw.numpy(), wdb.numpy()[0]]


def _dw_case(lib, B, S, Cc, k, glu, seed=0, span=0.0, strided=False):
    u, w, bias, dy = K.dwconv_inputs(B, S, Cc, k, bool(glu), seed, span)
    ref = K.dwconv_reference(u, w, bias, dy, bool(glu))
    R, W = B * S, (1 + glu) * Cc
    got = _dw_run(lib, u, w, bias, dy, B, S, Cc, k, glu)
    tag = f"dwconv B{B} S{S} C{Cc} k{k} glu{glu}"
    worst = 0.0
    for name, g, r in zip(("y", "du", "dw", "dbias"), got, (ref[0].reshape(R, Cc), ref[1].reshape(R, W), ref[2], ref[3])):
        worst = max(worst, check(f"{tag} {name}", g, r))
    if strided:      # strides change addresses only
        for name, a, b in zip(("y", "du", "dw", "dbias"), got, _dw_run(lib, u, w, bias, dy, B, S, Cc, k, glu, W + 5, W + 11)):
            assert np.array_equal(a, b), f"{tag} {name} strided"
    return got, ref, worst


@pytest.mark.parametrize("k", KS)
def test_depthwise_conv_every_kernel_size_frame_count_and_width(seld_lib, k):
    """k around the 8-tap chunk and at both ends of the range; S = 1, 2, k - 1, k, k + 1 (the kernel longer than, as long as and shorter than
    the clip) and 600 (five 128-frame tiles, the last ragged); C below, at and above the 64 lanes; with and without the GLU.  Every width at
    S = k + 1 and 600, three of them elsewhere."""
    worst = 0.0
    for S in sorted({1, 2, k - 1, k, k + 1, 600} - {0}):
        for Cc in (CS if S in (k + 1, 600) else [7, 65, 128]):
            for glu in (0, 1):
                if S == 600 and Cc in (7, 65) and glu == 0:
                    continue
                worst = max(worst, _dw_case(seld_lib, 2, S, Cc, k, glu, seed=k)[2])
    print(f"[worst] depthwise k={k}: {worst:.3e}")


@pytest.mark.parametrize("B,S,Cc,k,glu", [(2, 150, 65, 32, 1), (3, 33, 7, 8, 1), (2, 150, 128, 24, 0)])
def test_depthwise_conv_strides_and_a_second_run_give_the_same_bits(seld_lib, B, S, Cc, k, glu):
    got, _, _ = _dw_case(seld_lib, B, S, Cc, k, glu, seed=1, strided=True)
    u, w, bias, dy = K.dwconv_inputs(B, S, Cc, k, bool(glu), 1)
    for a, b in zip(got, _dw_run(seld_lib, u, w, bias, dy, B, S, Cc, k, glu)):
        assert np.array_equal(a, b)      # no atomics, a fixed summation order


@pytest.mark.parametrize("k,S,Cc", [(8, 40, 65), (64, 65, 64)])
def test_depthwise_conv_saturated_gates(seld_lib, k, S, Cc):
    """gates over [-40, 40], every 7th at exactly +-40: sigmoid'(40) = 4.2e-18 is lost by 1 - s on a rounded s.  The tensors at the project's bar,
    and the gate gradient at the saturated elements against its own value."""
    got, ref, _ = _dw_case(seld_lib, 2, S, Cc, k, 1, seed=2, span=40.0)
    u, _, _, _ = K.dwconv_inputs(2, S, Cc, k, True, 2, 40.0)
    sat = (np.abs(u[..., Cc:]) == 40.0).reshape(2 * S, Cc)
    assert sat.sum() > 100
    g2, r2 = got[1][:, Cc:][sat], ref[1].reshape(2 * S, 2 * Cc)[:, Cc:][sat]
    assert np.abs(r2).max() < 1e-15 and np.abs(r2).max() > 0
    assert np.abs(g2 - r2).max() <= 1e-4 * np.abs(r2).max()


@pytest.mark.parametrize("B,S,Cc,k", [(1030, 3, 7, 3), (8, 600, 128, 32)])
def test_depthwise_conv_second_stage_of_the_reduction(seld_lib, B, S, Cc, k):
    """1030 one-tile clips: more tiles than the 512 first-stage slots, so a workgroup walks several and the second stage folds 512 partials;
    8 x 600: 80 slots of ten tiles' worth each at the reference's width"""
    _dw_case(seld_lib, B, S, Cc, k, 1, seed=3)


def test_positional_add_and_head_permute(seld_lib):
    rng = np.random.default_rng(0)
    B, S, D, H, dk = 3, 61, 50, 5, 8
    x, enc = rng.standard_normal((B, S, D)).astype(np.float32), K.pos_table(S, D)
    xd = dev(x)
    assert seld_lib.seld_pos_add(ptr(xd), ptr(dev(enc)), B, S, D, _stream()) == 0
    w = rng.standard_normal((H, D, dk)).astype(np.float32)
    packed, back = torch.full((D, H, dk), float("nan"), device="cuda"), torch.full((H, D, dk), float("nan"), device="cuda")
    assert seld_lib.seld_head_permute(ptr(dev(w)), ptr(packed), H, D, dk, 0, _stream()) == 0
    assert seld_lib.seld_head_permute(ptr(packed), ptr(back), H, D, dk, 1, _stream()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(xd.cpu().numpy(), x + enc[None])
    assert np.array_equal(packed.cpu().numpy(), w.transpose(1, 0, 2)) and np.array_equal(back.cpu().numpy(), w)


# ---------------------------------------------------------------- the block and the stage
@pytest.mark.parametrize("name", sorted(K.STAGE_CASES))
def test_conformer_encoder_block_and_stage(name):
    """forward in training and in inference (they differ; inference follows the moving statistics the training step left), the input's and
    every variable's gradient"""
    from seld_amd import modules
    B, S, D, depth, cfg = K.STAGE_CASES[name]
    ref = K.stage_reference(B, S, D, depth, cfg, seed=3)
    tr, nt = ref["specs"]
    stage = (modules.conformer_encoder_stage if "depth" in cfg else modules.conformer_encoder_block)(cfg)((B, S, D))
    rt = stage.blocks[0].rt
    rt.finalize()
    assert [(n, s) for n, _, s in rt.variables] == tr and [(n, s) for n, _, s in rt.state_variables] == nt
    rt.params[:rt.n_params].copy_(torch.as_tensor(ref["w"]))
    rt.state[:rt.n_state].copy_(torch.as_tensor(ref["st"]))
    xd = dev(ref["x"].reshape(B * S, D))
    out = stage.forward(xd, B, True).cpu().numpy().copy()
    state = rt.state[:rt.n_state].cpu().numpy().copy()
    out_eval = stage.forward(xd, B, False).cpu().numpy().copy()
    rt.state[:rt.n_state].copy_(torch.as_tensor(ref["st"]))
    stage.forward(xd, B, True)
    dx = stage.backward(dev(ref["dy"].reshape(B * S, D)), B).cpu().numpy().copy()
    grads = rt.grads[:rt.n_params].cpu().numpy().copy()
    tag = f"conformer {name}"
    check(f"{tag} forward (training)", out, ref["out_train"].reshape(B * S, D))
    check(f"{tag} moving statistics", state, ref["new_state"])
    check(f"{tag} forward (inference)", out_eval, ref["out_eval"].reshape(B * S, D))
    assert np.abs(out - out_eval).max() > 1e-3 * np.abs(out).max()
    check(f"{tag} input gradient", dx, ref["dx"].reshape(B * S, D))
    off, biggest = 0, float(np.abs(ref["grad"]).max())
    for n, s in tr:
        kk = int(np.prod(s))
        _check_or_zero(f"{tag} grad {n}", grads[off:off + kk], ref["grad"][off:off + kk], biggest)
        off += kk


# ---------------------------------------------------------------- the model
@pytest.mark.parametrize("doa_loss", ["MSE", "MMSE"])
def test_train_step_with_a_conformer_encoder_stage(seldnet_config, doa_loss):
    """models.seldnet with FIRST = mother_stage (the arguments of test_train_step_with_a_mother_stage_first_block) and SECOND =
    conformer_encoder_stage: one test step and one train step against the fp64 oracle — variable list, outputs, both losses, every
    gradient, BatchNorm state, post-Adam weights — then a batch of 2 on the model built for 3"""
    from oracle import seldnet_oracle as O
    from seld_amd import losses, models, train
    from test_modules_gpu import STAGE_FIRST
    cfg = copy.deepcopy(seldnet_config)
    cfg["FIRST"], cfg["FIRST_ARGS"] = "mother_stage", copy.deepcopy(STAGE_FIRST)
    cfg["SECOND"] = "conformer_encoder_stage"
    cfg["SECOND_ARGS"] = {"depth": 2, "n_head": 4, "key_dim": 24, "kernel_size": 24, "multiplier": 2, "dropout_rate": 0}
    B, T_ = 3, 100
    in_shape = (B, T_, 64, 7)
    tr, nt = K.variable_specs(cfg, in_shape)
    w, st = K.random_weights(cfg, in_shape, seed=11)
    x, ys, yd = O.synthetic_batch(B, T_, seed=23)
    model = models.seldnet(in_shape, cfg)
    assert type(model).__name__ == "ComposedSeldNet"
    assert [(n, s) for n, _, s in model.variables] == tr and [(n, s) for n, _, s in model.state_variables] == nt
    assert sum(n.startswith("cf") for n, _ in tr) == 68 and not any(n.startswith("gru") for n, _ in tr)
    assert [n for n, _ in nt][-4:] == ["cf0.bn.moving_mean", "cf0.bn.moving_variance", "cf1.bn.moving_mean", "cf1.bn.moving_variance"]
    model.set_weights(w, st)
    f64 = lambda a: torch.tensor(a, dtype=torch.float64)
    sed_t, doa_t, _ = K.forward(cfg, O.unflatten(f64(w), tr), O.unflatten(f64(st), nt), f64(x), False)
    y_t, sl_t, dl_t = train.teststep(model, x, (ys, yd), losses.BinaryCrossentropy(), losses.get_doa_loss(doa_loss))
    check("conformer model teststep sed", y_t[0].cpu().numpy(), sed_t.numpy())
    check("conformer model teststep doa", y_t[1].cpu().numpy(), doa_t.numpy())
    ref = K.train_step(cfg, in_shape, w, st, x, ys, yd, doa_loss=doa_loss, loss_weight=(1.0, 1000.0), lr=1e-3, step=1)
    y_p, sl, dl = train.trainstep(model, x, (ys, yd), losses.BinaryCrossentropy(), losses.get_doa_loss(doa_loss), (1.0, 1000.0), train.Adam(1e-3))
    check("conformer model trainstep sed", y_p[0].cpu().numpy(), ref["sed"])
    check("conformer model trainstep doa", y_p[1].cpu().numpy(), ref["doa"])
    check("conformer model sloss", sl.cpu().numpy(), ref["sloss"])
    check("conformer model dloss", dl.cpu().numpy(), ref["dloss"])
    g = model.get_grads()
    biggest = np.abs(ref["grad"]).max()
    for n, off, sh in model.variables:
        k = int(np.prod(sh))
        _check_or_zero(f"conformer model grad {n}", g[off:off + k], ref["grad"][off:off + k], biggest)
    w1, st1 = model.get_weights()
    check("conformer model BN state", st1, ref["new_state"])
    big = np.abs(ref["grad"]) > 1e-3 * biggest
    assert np.abs(w1 - ref["new_w"])[big].max() <= 2e-3 * 1e-3 + 1e-7       # Adam's first step moves a weight by lr g / (|g| + eps)
    # a batch of 2 on the model built for 3
    y2 = model(x[:2], training=False)
    sed2, doa2, _ = K.forward(cfg, O.unflatten(f64(w1), tr), O.unflatten(f64(st1), nt), f64(x[:2]), False)
    assert tuple(y2[0].shape) == (2, T_ // 5, 12)
    check("conformer model batch of 2 sed", y2[0].cpu().numpy(), sed2.numpy())
    check("conformer model batch of 2 doa", y2[1].cpu().numpy(), doa2.numpy())
    y3, _, _ = train.trainstep(model, x[:2], (ys[:2], yd[:2]), losses.BinaryCrossentropy(), losses.get_doa_loss(doa_loss), (1.0, 1000.0), train.Adam(1e-3))
    assert tuple(y3[1].shape) == (2, T_ // 5, 36) and bool(torch.isfinite(y3[0]).all()) and np.isfinite(model.get_grads()).all()
