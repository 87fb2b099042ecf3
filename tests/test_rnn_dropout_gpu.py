"""The recurrent kinds under Keras dropout / recurrent_dropout on the device against the fp64 restatement tests/rnn_dropout_oracle.py at the
project's bar (helpers.check: max|d| / max|ref| <= 1e-4 per tensor; tests/test_rnn_dropout_cpu.py holds that a plain fp32 evaluation of every
case here stays within 5e-5): the LSTM dropout kernels (seld_rnn_lstm_drop_*: lstm.hip), the GRU dropout kernels per direction with the output
gradients as given (seld_rnn_gru_drop_*: gru.hip), seld_rnn_mask_rows, the blocks and stages built with dropout=True on the library's own draws,
and models.seldnet with SECOND = RNN_stage at dropout_rate 0.2 in a train step.

Buffers as in tests/test_rnn_gpu.py: every output sits in a NaN-filled allocation with a guard band in front and behind; inputs, bands
included, must hold their bits after the calls."""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch

import rnn_dropout_oracle as RD
import rnn_oracle as R
from helpers import check, dev, ptr, rel_err
from test_attention_gpu import _check_or_zero, _stream
from test_rnn_gpu import INVALID, UNSUPPORTED, _pad, _pair, _run_lstm, _win

pytestmark = pytest.mark.gpu

LSTM_KEYS = ("h", "c", "saved", "dgx")


# ---------------------------------------------------------------- the LSTM dropout kernels
def _run_lstm_drop(lib, ins, masks, B, S, nd=2, rows_for=None):
    """seld_rnn_lstm_drop_fwd + _bwd with the state masks [2][B,128] given -> {h, c, dgx: [per direction] [B,S,.], saved: [B*S,512]}"""
    Ba = rows_for or B
    R_, Ra = B * S, Ba * S
    gx = [_win(Ra, 512, _pad(ins["gx"][d], B, Ba)) for d in range(nd)]
    U = [_win(128, 512, ins["U"][d]) for d in range(nd)]
    rm = [_win(Ba, 128, np.concatenate([masks[d], np.zeros((Ba - B, 128), np.float32)])) for d in range(nd)]
    h, c, sv = ([_win(Ra, w) for _ in range(nd)] for w in (128, 128, 512))
    dh = [_win(Ra, 128, _pad(ins["dh"][d], B, Ba)) for d in range(nd)]
    dgx = [_win(Ra, 512) for _ in range(nd)]
    for w in gx + U + rm + dh:
        w.snapshot()
    assert lib.seld_rnn_lstm_drop_fwd(*_pair(gx, nd), *_pair(U, nd), *_pair(rm, nd), *_pair(h, nd), *_pair(c, nd), *_pair(sv, nd), B, S, 128,
                                      _stream()) == 0
    assert lib.seld_rnn_lstm_drop_bwd(*_pair(dh, nd), *_pair(c, nd), *_pair(sv, nd), *_pair(U, nd), *_pair(rm, nd), *_pair(dgx, nd), B, S, 128,
                                      _stream()) == 0
    torch.cuda.synchronize()
    for w in gx + U + rm + dh:
        w.assert_unchanged("gx / U / rm / dh")
    for w in h + c + sv + dgx:
        w.assert_band("h / c / saved / dgx")
        assert bool(torch.isnan(w.view[R_:]).all()), "rows of the larger batch were written"
    return {"h": [w.numpy()[:R_].reshape(B, S, 128) for w in h], "c": [w.numpy()[:R_].reshape(B, S, 128) for w in c],
            "saved": [w.numpy()[:R_] for w in sv], "dgx": [w.numpy()[:R_].reshape(B, S, 512) for w in dgx]}


@functools.lru_cache(maxsize=None)
def _lstm_case(B, S, rate):
    ins, masks = R.recurrence_inputs("lstm", B, S), R.gru_drop_masks(B, rate)
    return ins, masks, RD.lstm_reference(ins, masks)


def _check_lstm(tag, got, ref, dirs=(0, 1)):
    for k in LSTM_KEYS:
        for i, d in enumerate(dirs):
            check(f"{tag} {k}[{d}]", got[k][i].reshape(ref[k][d].shape), ref[k][d])


def _same_bits(tag, a, b, keys=LSTM_KEYS):
    for k in keys:
        for d in range(len(a[k])):
            assert np.isfinite(a[k][d]).all() and np.array_equal(a[k][d], b[k][d]), f"{tag}: {k}[{d}] differs"


@pytest.mark.parametrize("rate", RD.LSTM_RATES)
@pytest.mark.parametrize("B,S", RD.LSTM_DROP_CASES)
def test_lstm_dropout_forward_and_bptt_against_the_oracle(seld_lib, B, S, rate):
    """(1,1); B = 3 with S one below, at and one above the backward (8) and forward (16) staging chunks; 53: a ragged tail"""
    ins, masks, ref = _lstm_case(B, S, rate)
    _check_lstm(f"lstm dropout {(B, S, rate)}", _run_lstm_drop(seld_lib, ins, masks, B, S), ref)


def test_lstm_dropout_one_direction(seld_lib):
    B, S = R.UNI_CASE
    ins, masks, ref = _lstm_case(B, S, 0.5)
    _check_lstm(f"lstm dropout unidirectional {(B, S)}", _run_lstm_drop(seld_lib, ins, masks, B, S, nd=1), ref, dirs=(0,))


def test_lstm_dropout_with_all_ones_masks_is_the_undropped_recurrence_bit_for_bit(seld_lib):
    """the mask is folded into the register copy of U: times 1.0f the dropout form is the same recurrence; and a second run gives the same bits"""
    for B, S in ((3, 53), (3, 16)):
        ins = R.recurrence_inputs("lstm", B, S)
        _same_bits(f"all-ones masks {(B, S)}", _run_lstm(seld_lib, ins, B, S), _run_lstm_drop(seld_lib, ins, np.ones((2, B, 128), np.float32), B, S))
    ins, masks, _ = _lstm_case(3, 53, 0.5)
    _same_bits("a second run", _run_lstm_drop(seld_lib, ins, masks, 3, 53), _run_lstm_drop(seld_lib, ins, masks, 3, 53))


def test_lstm_dropout_every_clip_equals_that_clip_alone(seld_lib):
    B, S = RD.LSTM_BATCH_CASE
    ins, masks, ref = _lstm_case(B, S, 0.5)
    whole = _run_lstm_drop(seld_lib, ins, masks, B, S)
    _check_lstm(f"lstm dropout {(B, S)}", whole, ref)
    whole["saved"] = [a.reshape(B, S, 512) for a in whole["saved"]]
    for b in range(B):
        one = {k: ins[k][:, b:b + 1] if k != "U" else ins[k] for k in ins}
        alone = _run_lstm_drop(seld_lib, one, masks[:, b:b + 1], 1, S)
        for k in LSTM_KEYS:
            for d in (0, 1):
                assert np.array_equal(alone[k][d].reshape(whole[k][d][b].shape), whole[k][d][b]), f"clip {b}: {k}[{d}] depends on the batch around it"


def test_lstm_dropout_smaller_batch_on_buffers_sized_for_a_larger_one(seld_lib):
    B, S, Ba = RD.LSTM_SMALLER_BATCH
    ins, masks, ref = _lstm_case(B, S, 0.2)
    _check_lstm("lstm dropout b < B", _run_lstm_drop(seld_lib, ins, masks, B, S, rows_for=Ba), ref)


# ---------------------------------------------------------------- the GRU dropout kernels per direction
def _run_gru_drop(lib, ins, masks, B, S, nd=2, dh=None):
    """seld_rnn_gru_drop_fwd + _bwd -> {h, hm, saved, dgx, dgh}"""
    R_ = B * S
    gx = [_win(R_, 384, ins["gx"][d]) for d in range(nd)]
    U = [_win(128, 384, ins["U"][d]) for d in range(nd)]
    br = [_win(1, 384, ins["brec"][d]) for d in range(nd)]
    rm = [_win(B, 128, masks[d]) for d in range(nd)]
    h, hm, sv = ([_win(R_, w) for _ in range(nd)] for w in (128, 128, 512))
    wdh = [_win(R_, 128, (ins["dh"] if dh is None else dh)[d]) for d in range(nd)]
    dgx, dgh = [_win(R_, 384) for _ in range(nd)], [_win(R_, 384) for _ in range(nd)]
    for w in gx + U + br + rm + wdh:
        w.snapshot()
    assert lib.seld_rnn_gru_drop_fwd(*_pair(gx, nd), *_pair(U, nd), *_pair(br, nd), *_pair(rm, nd), *_pair(h, nd), *_pair(hm, nd), *_pair(sv, nd),
                                     B, S, 128, _stream()) == 0
    assert lib.seld_rnn_gru_drop_bwd(*_pair(wdh, nd), *_pair(hm, nd), *_pair(sv, nd), *_pair(U, nd), *_pair(rm, nd), *_pair(dgx, nd),
                                     *_pair(dgh, nd), B, S, 128, _stream()) == 0
    torch.cuda.synchronize()
    for w in gx + U + br + rm + wdh:
        w.assert_unchanged("GRU input")
    for w in h + hm + sv + dgx + dgh:
        w.assert_band("GRU output")
    return {"h": [w.numpy().reshape(B, S, 128) for w in h], "hm": [w.numpy().reshape(B, S, 128) for w in hm], "saved": [w.numpy() for w in sv],
            "dgx": [w.numpy().reshape(B, S, 384) for w in dgx], "dgh": [w.numpy().reshape(B, S, 384) for w in dgh]}


@pytest.mark.parametrize("B,S", R.GRU_DROP_CASES + R.GRU_DROP_AT_CHUNKS)
def test_gru_dropout_per_direction_against_the_oracle(seld_lib, B, S):
    ins, masks = R.recurrence_inputs("gru", B, S), R.gru_drop_masks(B, R.GRU_DROP_RATE)
    R.gru_compare(f"rnn gru dropout {(B, S)}", _run_gru_drop(seld_lib, ins, masks, B, S), R.gru_reference(ins, rec_mask=masks), 1e-4)


def test_gru_dropout_one_direction(seld_lib):
    B, S = R.UNI_CASE
    ins, masks = R.recurrence_inputs("gru", B, S), R.gru_drop_masks(B, R.GRU_DROP_RATE)
    R.gru_compare("rnn gru dropout unidirectional", _run_gru_drop(seld_lib, ins, masks, B, S, nd=1), R.gru_reference(ins, dirs=(0,), rec_mask=masks), 1e-4)


def test_gru_dropout_reproduces_the_mul_merged_entries_bit_for_bit(seld_lib):
    """dh_f = dout h_b, dh_b = dout h_f (formed here in fp32, as seld_k_gru_drop_bwd's kernel forms them) -> its dgx / dgh; the forward is the
    same kernel on the caller's stream"""
    lib = seld_lib
    B, S = 3, 33
    ins, masks = R.recurrence_inputs("gru", B, S), R.gru_drop_masks(B, R.GRU_DROP_RATE)
    R_ = B * S
    t = lambda a, c: dev(np.asarray(a).reshape(-1, c))
    gx, U, br = ([t(ins[k][d], 384) for d in (0, 1)] for k in ("gx", "U", "brec"))
    rm = [t(masks[d], 128) for d in (0, 1)]
    nan = lambda w, n=2: [torch.full((R_, w), float("nan"), device="cuda") for _ in range(n)]
    p2 = lambda ts: (ptr(ts[0]), ptr(ts[1]))
    h, hm, sv = nan(128), nan(128), nan(512)
    assert lib.seld_k_gru_drop_fwd(*p2(gx), *p2(U), *p2(br), *p2(rm), *p2(h), *p2(hm), *p2(sv), B, S, 128) == 0
    dout = t(ins["dh"][0], 128)
    a = nan(384, 4)
    assert lib.seld_k_gru_drop_bwd(ptr(dout), *p2(h), *p2(hm), *p2(sv), *p2(U), *p2(rm), *p2(a[0:2]), *p2(a[2:4]), B, S, 128) == 0
    h2, hm2, sv2 = nan(128), nan(128), nan(512)
    assert lib.seld_rnn_gru_drop_fwd(*p2(gx), *p2(U), *p2(br), *p2(rm), *p2(h2), *p2(hm2), *p2(sv2), B, S, 128, _stream()) == 0
    dh = [dout * h[1], dout * h[0]]
    b = nan(384, 4)
    assert lib.seld_rnn_gru_drop_bwd(*p2(dh), *p2(hm2), *p2(sv2), *p2(U), *p2(rm), *p2(b[0:2]), *p2(b[2:4]), B, S, 128, _stream()) == 0
    torch.cuda.synchronize()
    for name, x, y in zip(("h_f", "h_b", "hm_f", "hm_b", "saved_f", "saved_b", "dgx_f", "dgx_b", "dgh_f", "dgh_b"), h + hm + sv + a, h2 + hm2 + sv2 + b):
        assert bool(torch.isfinite(x).all()) and torch.equal(x, y), name


# ---------------------------------------------------------------- seld_rnn_mask_rows
def _off(w, nbytes):
    return ctypes.c_void_p(w.view.data_ptr() + nbytes)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("B,S,F", [(2, 3, 40), (3, 5, 128)])
def test_mask_rows_on_a_stream_equals_the_null_stream_entry(seld_lib, B, S, F, accumulate):
    rng = np.random.default_rng([B, S, F, accumulate])
    x, m, prev = R.f32(rng.standard_normal((B * S, F))), R.f32(rng.standard_normal((B, F))), R.f32(rng.standard_normal((B * S, F)))
    wx, wm = _win(B * S, F, x), _win(B, F, m)
    a, b = _win(B * S, F, prev), _win(B * S, F, prev)
    wx.snapshot(); wm.snapshot()
    assert seld_lib.seld_k_mask_rows(wx.ptr(), wm.ptr(), a.ptr(), B * S, S, F, accumulate) == 0
    assert seld_lib.seld_rnn_mask_rows(wx.ptr(), wm.ptr(), b.ptr(), B * S, S, F, accumulate, _stream()) == 0
    torch.cuda.synchronize()
    wx.assert_unchanged("in"); wm.assert_unchanged("mask")
    a.assert_band("out"); b.assert_band("out")
    assert torch.equal(a.view, b.view)
    want = x.astype(np.float64) * np.repeat(m, S, axis=0) + (prev if accumulate else 0)
    check(f"mask_rows {(B, S, F, accumulate)}", b.numpy(), want, 1e-6)
    for bad in ((None, wm.ptr(), b.ptr(), B * S, S, F), (wx.ptr(), None, b.ptr(), B * S, S, F), (wx.ptr(), wm.ptr(), None, B * S, S, F),
                (wx.ptr(), wm.ptr(), b.ptr(), 0, S, F), (wx.ptr(), wm.ptr(), b.ptr(), B * S, 0, F), (wx.ptr(), wm.ptr(), b.ptr(), B * S, S, F - 2),
                (_off(wx, 4), wm.ptr(), b.ptr(), B * S, S, F)):
        assert seld_lib.seld_rnn_mask_rows(*bad, accumulate, _stream()) == INVALID
    torch.cuda.synchronize()
    assert torch.equal(a.view, b.view), "a refused call wrote"


# ---------------------------------------------------------------- refusals
def test_dropout_recurrence_refusals_write_nothing(seld_lib):
    """each of the four entries: units != 128 -> UNSUPPORTED before any other check; every pointer in turn NULL (a required one missing, a
    half-given second direction, or one direction with *_b arguments), B = 0, S = 0 -> INVALID; nothing is enqueued"""
    lib, B, S = seld_lib, 2, 5
    st = _stream()
    w = lambda rows, cols: [_win(rows, cols), _win(rows, cols)]
    gxl, Ul, hl, cl, svl, dgl = w(B * S, 512), w(128, 512), w(B * S, 128), w(B * S, 128), w(B * S, 512), w(B * S, 512)
    gxg, Ug, bg, hmg, dgg, dhg = w(B * S, 384), w(128, 384), w(1, 384), w(B * S, 128), w(B * S, 384), w(B * S, 384)
    rm = w(B, 128)
    p = lambda ws: [ws[0].ptr(), ws[1].ptr()]
    calls = ((lib.seld_rnn_lstm_drop_fwd, p(gxl) + p(Ul) + p(rm) + p(hl) + p(cl) + p(svl)),
             (lib.seld_rnn_lstm_drop_bwd, p(hl) + p(cl) + p(svl) + p(Ul) + p(rm) + p(dgl)),
             (lib.seld_rnn_gru_drop_fwd, p(gxg) + p(Ug) + p(bg) + p(rm) + p(hl) + p(hmg) + p(svl)),
             (lib.seld_rnn_gru_drop_bwd, p(cl) + p(hmg) + p(svl) + p(Ug) + p(rm) + p(dgg) + p(dhg)))
    for fn, args in calls:
        assert fn(*args, B, S, 64, st) == UNSUPPORTED
        assert fn(*([None] * len(args)), 0, 0, 64, st) == UNSUPPORTED
        for i in range(len(args)):
            assert fn(*(args[:i] + [None] + args[i + 1:]), B, S, 128, st) == INVALID, (fn.__name__, i)
        one = [a if i % 2 == 0 else None for i, a in enumerate(args)]      # one direction: every *_b argument NULL
        for i in range(0, len(args), 2):
            assert fn(*(one[:i] + [None] + one[i + 1:]), B, S, 128, st) == INVALID, (fn.__name__, i)
        assert fn(*args, 0, S, 128, st) == INVALID and fn(*args, B, 0, 128, st) == INVALID
        assert fn(*one, 0, S, 128, st) == INVALID and fn(*one, B, 0, 128, st) == INVALID
    torch.cuda.synchronize()
    for ws in (gxl, Ul, hl, cl, svl, dgl, gxg, Ug, bg, hmg, dgg, dhg, rm):
        for x in ws:
            assert bool(torch.isnan(x.buf).all()), "a refused call wrote"


# ---------------------------------------------------------------- blocks and stages on the library's draws
@functools.lru_cache(maxsize=None)
def _stage_ref(name, step):
    kind, B, S, D, cfg = RD.STAGE_CASES[name]
    return RD.stage_reference(kind, B, S, D, cfg, RD.STAGE_SEED, step)


def _build(kind, cfg, S, D, B, w):
    from seld_amd import modules
    stage = modules._build_second(kind, None, cfg, S, D, B, dropout=True)
    rt = stage.blocks[0].rt
    rt.finalize()
    rt.params[:rt.n_params].copy_(torch.as_tensor(w))
    return stage, rt


@pytest.mark.parametrize("name", sorted(RD.STAGE_CASES))
def test_blocks_and_stages_train_under_dropout(name):
    """the training forward at the first two dropout steps, the input's and every variable's gradient against the oracle on the library's draws;
    inference is the rate-0 block's bit for bit; the masks matter, change from step to step and repeat when the step does"""
    kind, B, S, D, cfg = RD.STAGE_CASES[name]
    ref, ref1 = _stage_ref(name, 0), _stage_ref(name, 1)
    tr = ref["specs"]
    stage, rt = _build(kind, cfg, S, D, B, ref["w"])
    plain, _ = _build(kind, dict(copy.deepcopy(cfg), dropout_rate=0.0), S, D, B, ref["w"])
    assert [(n, s) for n, _, s in rt.variables] == tr and not rt.state_variables
    assert [b.drop.base for b in stage.blocks] == [4096 + 32 * i for i in range(len(stage.blocks))]
    xd, dy = dev(ref["x"].reshape(B * S, D)), dev(ref["dy"].reshape(B * S, -1))
    x0 = xd.clone()
    out_eval = stage.forward(xd, B, False).clone()
    assert torch.equal(out_eval, plain.forward(xd, B, False)), "inference is not the rate-0 block's"
    assert rt.dropout_step == 0

    def train():
        out = stage.forward(xd, B, True).clone()
        dx = stage.backward(dy, B).clone()
        return out, dx, rt.grads[:rt.n_params].clone()
    out, dx, grads = train()
    assert rt.dropout_cur == 0 and rt.dropout_step == 1
    out1, _, _ = train()
    rt.dropout_step = 0
    again = train()
    assert torch.equal(xd, x0)
    tag = f"RNN dropout {name}"
    check(f"{tag} forward", out.cpu().numpy(), ref["out"].reshape(B * S, -1))
    check(f"{tag} forward, next step", out1.cpu().numpy(), ref1["out"].reshape(B * S, -1))
    check(f"{tag} input gradient", dx.cpu().numpy(), ref["dx"].reshape(B * S, D))
    g = grads.cpu().numpy()
    off, biggest = 0, float(np.abs(ref["grad"]).max())
    for n, s in tr:
        kk = int(np.prod(s))
        _check_or_zero(f"{tag} grad {n}", g[off:off + kk], ref["grad"][off:off + kk], biggest)
        off += kk
    assert rel_err(out.cpu().numpy(), out_eval.cpu().numpy()) > 1e-6, "the masks do not matter"
    assert rel_err(out1.cpu().numpy(), out.cpu().numpy()) > 1e-6, "the next step drew the same masks"
    for what, a, b in zip(("forward", "input gradient", "gradients"), (out, dx, grads), again):
        assert torch.equal(a, b), f"{what}: the same dropout step gives other bits"


# ---------------------------------------------------------------- the model
def test_train_step_with_an_rnn_stage_under_dropout(seldnet_config):
    """models.seldnet with SECOND = RNN_stage (GRU, 'ave', depth 2) at dropout_rate 0.2: a test_step equals the rate-0 model's, given the same
    weights; then one train step — both outputs, both losses and every gradient — against the oracle at dropout step 0"""
    from oracle import seldnet_oracle as O
    from seld_amd import losses, models, train
    from test_modules_gpu import STAGE_FIRST
    cfg = RD.model_case(seldnet_config, STAGE_FIRST)
    cfg0 = RD.model_case(seldnet_config, STAGE_FIRST, rate=0.0)
    B, T_ = R.MODEL_INPUT[:2]
    tr, nt = R.variable_specs(cfg, R.MODEL_INPUT)
    w, st = R.random_weights(cfg, R.MODEL_INPUT, seed=11)
    x, ys, yd = O.synthetic_batch(B, T_, seed=23)
    model, model0 = models.seldnet(R.MODEL_INPUT, cfg), models.seldnet(R.MODEL_INPUT, cfg0)
    assert type(model).__name__ == "ComposedSeldNet"
    assert [(n, s) for n, _, s in model.variables] == tr and [(n, s) for n, _, s in model.state_variables] == nt
    assert [b.drop.rate for b in model.second.blocks] == [float(np.float32(0.2))] * 2 and [b.drop.rate for b in model0.second.blocks] == [0.0] * 2
    model.set_weights(w, st)
    model0.set_weights(w, st)
    bce, mse, lw = losses.BinaryCrossentropy(), losses.get_doa_loss("MSE"), (1.0, 1000.0)
    (ya, sla, dla), (yb, slb, dlb) = train.teststep(model, x, (ys, yd), bce, mse), train.teststep(model0, x, (ys, yd), bce, mse)
    for k, a, b in (("sed", ya[0], yb[0]), ("doa", ya[1], yb[1]), ("sloss", sla, slb), ("dloss", dla, dlb)):
        assert torch.equal(a, b), f"test_step {k}: the rate-{0.2} model's differs from the rate-0 model's"
    assert model.rt.dropout_step == 0
    ref = RD.train_step(cfg, R.MODEL_INPUT, w, st, x, ys, yd, dropout_step=0, doa_loss="MSE", loss_weight=lw)
    y_p, sl, dl = train.trainstep(model, x, (ys, yd), bce, mse, lw, train.Adam(1e-3))
    assert model.rt.dropout_step == 1
    check("rnn dropout model trainstep sed", y_p[0].cpu().numpy(), ref["sed"])
    check("rnn dropout model trainstep doa", y_p[1].cpu().numpy(), ref["doa"])
    check("rnn dropout model sloss", sl.cpu().numpy(), ref["sloss"])
    check("rnn dropout model dloss", dl.cpu().numpy(), ref["dloss"])
    g = model.get_grads()
    biggest = np.abs(ref["grad"]).max()
    for n, off, sh in model.variables:
        k = int(np.prod(sh))
        _check_or_zero(f"rnn dropout model grad {n}", g[off:off + k], ref["grad"][off:off + k], biggest)
    assert rel_err(y_p[0].cpu().numpy(), ya[0].cpu().numpy()) > 1e-6, "the masks do not matter"
