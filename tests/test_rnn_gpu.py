"""The recurrent block of the reference (modules.RNN_block / RNN_stage, modules.py:64-83, 322-347) on the device against the fp64 restatement
tests/rnn_oracle.py at the project's bar (helpers.check: max|d| / max|ref| <= 1e-4 per tensor; tests/test_rnn_cpu.py holds that a plain fp32 evaluation of
every case here stays within 5e-5): the LSTM recurrence kernels (seld_rnn_lstm_*: seld_amd/csrc/lstm.hip), the GRU recurrence per direction with the
output gradients as given (seld_rnn_gru_*: gru.hip), Bidirectional's merges (seld_rnn_merge_*), seld_amd.modules.RNNBlock / RNNStage, and
models.seldnet with SECOND = RNN_stage in a train step.

Every output sits in a NaN-filled allocation with a guard band in front and behind (512 floats: the kernels move float4, so the windows stay 16-byte
aligned); inputs, bands included, must hold their bits after the calls."""
import functools

import numpy as np
import pytest
import torch

import rnn_oracle as R
from helpers import check, dev, ptr
from test_attention_gpu import _Window, _check_or_zero, _stream

pytestmark = pytest.mark.gpu

BAND = 512
UNSUPPORTED, INVALID = -2, -1


def _win(rows, cols, data=None):
    return _Window(rows, cols, None, None, BAND, BAND, data)


def _pair(ws, nd):
    """(forward, backward) pointers of a per-direction window list; one direction: (pointer, NULL)"""
    return (ws[0].ptr(), ws[1].ptr() if nd == 2 else None)


@functools.lru_cache(maxsize=None)
def _lstm_case(B, S, scale=1.0):
    ins = R.recurrence_inputs("lstm", B, S, scale)
    return ins, R.lstm_reference(ins)


@functools.lru_cache(maxsize=None)
def _gru_case(B, S):
    ins = R.recurrence_inputs("gru", B, S)
    return ins, R.gru_reference(ins)


def _pad(a, B, Ba):
    """[B, S, C] -> [Ba * S, C] rows (zeros behind the batch that runs)"""
    a = np.asarray(a)
    S, C_ = a.shape[1], a.shape[2]
    return np.concatenate([a.reshape(B * S, C_), np.zeros(((Ba - B) * S, C_), a.dtype)]) if Ba > B else a.reshape(B * S, C_)


def _run_lstm(lib, ins, B, S, nd=2, save=True, rows_for=None):
    """seld_rnn_lstm_fwd (+ _bwd when save) -> {h, c, dgx: [per direction] numpy [B,S,.]}"""
    Ba = rows_for or B
    R_, Ra = B * S, Ba * S
    gx = [_win(Ra, 512, _pad(ins["gx"][d], B, Ba)) for d in range(nd)]
    U = [_win(128, 512, ins["U"][d]) for d in range(nd)]
    h, c, sv = ([_win(Ra, w) for _ in range(nd)] for w in (128, 128, 512))
    for w in gx + U:
        w.snapshot()
    none = (None, None)
    rc = lib.seld_rnn_lstm_fwd(*_pair(gx, nd), *_pair(U, nd), *_pair(h, nd), *(_pair(c, nd) if save else none), *(_pair(sv, nd) if save else none),
                             B, S, 128, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    for w in gx + U:
        w.assert_unchanged("gx / U")
    for w in h + c + sv:
        w.assert_band("h / c / saved")
    out = {"h": [w.numpy()[:R_].reshape(B, S, 128) for w in h]}
    for w in h + c + sv:
        assert bool(torch.isnan(w.view[R_:]).all())                     # rows of the larger batch stay untouched
        assert save or w in h or bool(torch.isnan(w.view).all())        # nothing is saved when saving is not asked for
    if not save:
        return out
    out["c"] = [w.numpy()[:R_].reshape(B, S, 128) for w in c]
    out["saved"] = [w.numpy()[:R_] for w in sv]
    dh = [_win(Ra, 128, _pad(ins["dh"][d], B, Ba)) for d in range(nd)]
    dgx = [_win(Ra, 512) for _ in range(nd)]
    for w in dh + c + sv + U:
        w.snapshot()
    rc = lib.seld_rnn_lstm_bwd(*_pair(dh, nd), *_pair(c, nd), *_pair(sv, nd), *_pair(U, nd), *_pair(dgx, nd), B, S, 128, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    for w in dh + c + sv + U:
        w.assert_unchanged("dh / c / saved / U")
    for w in dgx:
        w.assert_band("dgx")
        assert bool(torch.isnan(w.view[R_:]).all())
    out["dgx"] = [w.numpy()[:R_].reshape(B, S, 512) for w in dgx]
    return out


def _check_lstm(tag, got, ref, dirs=(0, 1)):
    for k in ("h", "c", "dgx"):
        for i, d in enumerate(dirs):
            check(f"{tag} {k}[{d}]", got[k][i], ref[k][d])


@pytest.mark.parametrize("B,S", R.LSTM_CASES)
def test_lstm_forward_and_bptt_against_the_oracle(seld_lib, B, S):
    """(1,1), (2,10), (3,60); S one below, at and one above each kernel's staging chunk (16 forward steps, 8 backward); S = 53: three forward and six
    backward chunks and a ragged tail"""
    ins, ref = _lstm_case(B, S)
    got = _run_lstm(seld_lib, ins, B, S)
    _check_lstm(f"lstm {(B, S)}", got, ref)
    i, f, g, o = (got["saved"][0].reshape(B * S, 128, 4)[..., k] for k in range(4))      # the four activations, per unit
    assert (i > 0).all() and (i < 1).all() and (f > 0).all() and (o > 0).all() and (np.abs(g) <= 1).all()


def test_lstm_one_direction(seld_lib):
    B, S = R.UNI_CASE
    ins = R.recurrence_inputs("lstm", B, S)
    ref = R.lstm_reference(ins, dirs=(0,))
    _check_lstm(f"lstm unidirectional {(B, S)}", _run_lstm(seld_lib, ins, B, S, nd=1), {k: {0: v[0]} for k, v in ref.items()}, dirs=(0,))


def test_lstm_same_bits_without_saving_and_on_a_second_run(seld_lib):
    B, S = 3, 60
    ins, _ = _lstm_case(B, S)
    a, b = _run_lstm(seld_lib, ins, B, S), _run_lstm(seld_lib, ins, B, S)
    for k in ("h", "c", "saved", "dgx"):
        for d in (0, 1):
            assert np.array_equal(a[k][d], b[k][d]), f"{k}[{d}]: a second run gives other bits"
    n = _run_lstm(seld_lib, ins, B, S, save=False)
    for d in (0, 1):
        assert np.array_equal(a["h"][d], n["h"][d]), f"h[{d}]: saved = NULL changes h"


def test_lstm_smaller_batch_on_buffers_sized_for_a_larger_one(seld_lib):
    B, S = 2, 17
    ins, ref = _lstm_case(B, S)
    _check_lstm("lstm b < B", _run_lstm(seld_lib, ins, B, S, rows_for=3), ref)


def test_lstm_saturated_gates_stay_finite(seld_lib):
    B, S, scale = R.SATURATED
    ins, ref = _lstm_case(B, S, scale)
    assert np.abs(ins["gx"]).max() > 30
    got = _run_lstm(seld_lib, ins, B, S)
    for k in ("h", "c", "saved", "dgx"):
        assert all(np.isfinite(a).all() for a in got[k]), k
    _check_lstm(f"lstm x{scale}", got, ref)


def test_recurrence_refusals_write_nothing(seld_lib):
    """units != 128 -> UNSUPPORTED before any other check; a NULL U_f, a half-given backward side, S = 0 -> INVALID; nothing is enqueued"""
    lib, B, S = seld_lib, 2, 5
    ins = R.recurrence_inputs("lstm", B, S)
    gx = [_win(B * S, 512, ins["gx"][d]) for d in (0, 1)]
    U = [_win(128, 512, ins["U"][d]) for d in (0, 1)]
    outs = [_win(B * S, w) for w in (128, 128, 128, 128, 512, 512, 512, 512)]      # h_f h_b c_f c_b sv_f sv_b dgx_f dgx_b
    h, c, sv, dgx = outs[0:2], outs[2:4], outs[4:6], outs[6:8]
    p = lambda ws: _pair(ws, 2)
    st = _stream()
    assert lib.seld_rnn_lstm_fwd(*p(gx), *p(U), *p(h), *p(c), *p(sv), B, S, 64, st) == UNSUPPORTED
    assert lib.seld_rnn_lstm_fwd(None, None, None, None, None, None, None, None, None, None, 0, 0, 64, st) == UNSUPPORTED
    assert lib.seld_rnn_lstm_fwd(*p(gx), None, U[1].ptr(), *p(h), *p(c), *p(sv), B, S, 128, st) == INVALID
    assert lib.seld_rnn_lstm_fwd(*p(gx), *p(U), *p(h), *p(c), *p(sv), B, 0, 128, st) == INVALID
    assert lib.seld_rnn_lstm_fwd(*p(gx), *p(U), *p(h), *p(c), *p(sv), 0, S, 128, st) == INVALID
    assert lib.seld_rnn_lstm_fwd(gx[0].ptr(), None, *p(U), *p(h), *p(c), *p(sv), B, S, 128, st) == INVALID       # one direction with *_b arguments
    assert lib.seld_rnn_lstm_fwd(*p(gx), *p(U), h[0].ptr(), None, *p(c), *p(sv), B, S, 128, st) == INVALID
    assert lib.seld_rnn_lstm_bwd(*p(h), *p(c), *p(sv), *p(U), *p(dgx), B, S, 64, st) == UNSUPPORTED
    assert lib.seld_rnn_lstm_bwd(*p(h), *p(c), *p(sv), None, U[1].ptr(), *p(dgx), B, S, 128, st) == INVALID
    assert lib.seld_rnn_lstm_bwd(*p(h), *p(c), *p(sv), *p(U), dgx[0].ptr(), None, B, S, 128, st) == INVALID     # a half-given backward side
    assert lib.seld_rnn_lstm_bwd(*p(h), c[0].ptr(), None, *p(sv), *p(U), *p(dgx), B, S, 128, st) == INVALID
    assert lib.seld_rnn_lstm_bwd(h[0].ptr(), None, *p(c), *p(sv), *p(U), *p(dgx), B, S, 128, st) == INVALID
    assert lib.seld_rnn_lstm_bwd(*p(h), *p(c), *p(sv), *p(U), *p(dgx), B, 0, 128, st) == INVALID
    g = [_win(B * S, 384) for _ in range(6)]      # gx_f gx_b dgx_f dgx_b dgh_f dgh_b of the GRU entries
    Ug, bg = [_win(128, 384) for _ in (0, 1)], [_win(1, 384) for _ in (0, 1)]
    assert lib.seld_rnn_gru_fwd(*p(g[0:2]), *p(Ug), *p(bg), *p(h), *p(sv), B, S, 64, st) == UNSUPPORTED
    assert lib.seld_rnn_gru_fwd(*p(g[0:2]), None, Ug[1].ptr(), *p(bg), *p(h), *p(sv), B, S, 128, st) == INVALID
    assert lib.seld_rnn_gru_fwd(*p(g[0:2]), *p(Ug), *p(bg), *p(h), *p(sv), B, 0, 128, st) == INVALID
    assert lib.seld_rnn_gru_bwd(*p(c), *p(h), *p(sv), *p(Ug), *p(g[2:4]), *p(g[4:6]), B, S, 64, st) == UNSUPPORTED
    assert lib.seld_rnn_gru_bwd(*p(c), *p(h), *p(sv), *p(Ug), *p(g[2:4]), g[4].ptr(), None, B, S, 128, st) == INVALID
    assert lib.seld_rnn_gru_bwd(*p(c), *p(h), *p(sv), *p(Ug), *p(g[2:4]), *p(g[4:6]), B, 0, 128, st) == INVALID
    torch.cuda.synchronize()
    for w in outs + g + Ug + bg:
        assert bool(torch.isnan(w.buf).all()), "a refused call wrote"


# ---------------------------------------------------------------- Bidirectional's merges
@pytest.mark.parametrize("rows", [1, 257])
@pytest.mark.parametrize("units", [128, 3])
@pytest.mark.parametrize("mode", R.MERGES)
def test_rnn_merge_forward_and_backward(seld_lib, mode, units, rows):
    """units 128: the float4 kernels; units 3: the scalar ones; 257 rows: more than one workgroup and a ragged last one"""
    from seld_amd import _lib
    hf, hb, dout = R.merge_inputs(rows, units, mode)
    y, ga, gb = R.merge_reference(hf, hb, dout, mode)
    m, wd = _lib.SELD_MERGE[mode], dout.shape[1]
    wf, wb, wdo = _win(rows, units, hf), _win(rows, units, hb), _win(rows, wd, dout)
    wy, wga, wgb = _win(rows, wd), _win(rows, units), _win(rows, units)
    for w in (wf, wb, wdo):
        w.snapshot()
    assert seld_lib.seld_rnn_merge_fwd(wf.ptr(), wb.ptr(), wy.ptr(), rows, units, m, _stream()) == 0
    needs_h = mode == "mul"
    assert seld_lib.seld_rnn_merge_bwd(wdo.ptr(), wf.ptr() if needs_h else None, wb.ptr() if needs_h else None, wga.ptr(), wgb.ptr(), rows, units, m,
                                         _stream()) == 0
    torch.cuda.synchronize()
    for w in (wf, wb, wdo):
        w.assert_unchanged("merge input")
    for name, w, ref in (("out", wy, y), ("dh_f", wga, ga), ("dh_b", wgb, gb)):
        w.assert_band(name)
        check(f"merge {mode} {(rows, units)} {name}", w.numpy(), ref)


def test_rnn_merge_refuses_an_unknown_mode(seld_lib):
    w = [_win(4, 128) for _ in range(5)]
    for mode in (-1, 4):
        assert seld_lib.seld_rnn_merge_fwd(w[0].ptr(), w[1].ptr(), w[2].ptr(), 4, 128, mode, _stream()) == INVALID
        assert seld_lib.seld_rnn_merge_bwd(w[2].ptr(), w[0].ptr(), w[1].ptr(), w[3].ptr(), w[4].ptr(), 4, 128, mode, _stream()) == INVALID
    assert seld_lib.seld_rnn_merge_bwd(w[2].ptr(), None, w[1].ptr(), w[3].ptr(), w[4].ptr(), 4, 128, 0, _stream()) == INVALID      # mul reads h
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(x.buf).all()) for x in w)


# ---------------------------------------------------------------- the GRU recurrence per direction
def _run_gru(lib, ins, B, S, nd=2, dh=None):
    """seld_rnn_gru_fwd + _bwd -> {h, dgx, dgh}"""
    R_ = B * S
    gx = [_win(R_, 384, ins["gx"][d]) for d in range(nd)]
    U = [_win(128, 384, ins["U"][d]) for d in range(nd)]
    br = [_win(1, 384, ins["brec"][d]) for d in range(nd)]
    h, sv = [_win(R_, 128) for _ in range(nd)], [_win(R_, 512) for _ in range(nd)]
    assert lib.seld_rnn_gru_fwd(*_pair(gx, nd), *_pair(U, nd), *_pair(br, nd), *_pair(h, nd), *_pair(sv, nd), B, S, 128, _stream()) == 0
    wdh = [_win(R_, 128, (ins["dh"] if dh is None else dh)[d]) for d in range(nd)]
    dgx, dgh = [_win(R_, 384) for _ in range(nd)], [_win(R_, 384) for _ in range(nd)]
    torch.cuda.synchronize()
    for w in gx + U + br + h + sv + wdh:
        w.snapshot()
    assert lib.seld_rnn_gru_bwd(*_pair(wdh, nd), *_pair(h, nd), *_pair(sv, nd), *_pair(U, nd), *_pair(dgx, nd), *_pair(dgh, nd), B, S, 128,
                                  _stream()) == 0
    torch.cuda.synchronize()
    for w in gx + U + br + h + sv + wdh:
        w.assert_unchanged("GRU input")
    for w in h + sv + dgx + dgh:
        w.assert_band("GRU output")
    return {"h": [w.numpy().reshape(B, S, 128) for w in h], "dgx": [w.numpy().reshape(B, S, 384) for w in dgx],
            "dgh": [w.numpy().reshape(B, S, 384) for w in dgh]}


@pytest.mark.parametrize("B,S", R.GRU_DH_CASES)
def test_rnn_gru_with_independent_output_gradients(seld_lib, B, S):
    ins, ref = _gru_case(B, S)
    got = _run_gru(seld_lib, ins, B, S)
    for k in ("h", "dgx", "dgh"):
        for d in (0, 1):
            check(f"rnn_gru {(B, S)} {k}[{d}]", got[k][d], ref[k][d])


def test_rnn_gru_one_direction(seld_lib):
    B, S = R.UNI_CASE
    ins = R.recurrence_inputs("gru", B, S)
    ref = R.gru_reference(ins, dirs=(0,))
    got = _run_gru(seld_lib, ins, B, S, nd=1)
    for k in ("h", "dgx", "dgh"):
        check(f"rnn_gru unidirectional {k}", got[k][0], ref[k][0])


def test_rnn_gru_reproduces_the_mul_merged_entry_bit_for_bit(seld_lib):
    """dh_f = dout h_b, dh_b = dout h_f (formed here in fp32, as the kernel of seld_m_gru_bwd forms them) -> the dgx / dgh of seld_m_gru_bwd"""
    lib = seld_lib
    B, S = R.GRU_MUL_CASE
    ins = R.recurrence_inputs("gru", B, S)
    R_ = B * S
    t = lambda a, c: dev(np.asarray(a).reshape(-1, c))
    gx, U, br = ([t(ins[k][d], 384) for d in (0, 1)] for k in ("gx", "U", "brec"))
    h, sv = [torch.full((R_, 128), float("nan"), device="cuda") for _ in (0, 1)], [torch.full((R_, 512), float("nan"), device="cuda") for _ in (0, 1)]
    p2 = lambda ts: (ptr(ts[0]), ptr(ts[1]))
    assert lib.seld_m_gru_fwd(*p2(gx), *p2(U), *p2(br), *p2(h), *p2(sv), None, B, S, 128, _stream()) == 0
    dout = t(ins["dh"][0], 128)
    a = [torch.full((R_, 384), float("nan"), device="cuda") for _ in range(4)]
    assert lib.seld_m_gru_bwd(ptr(dout), *p2(h), *p2(sv), *p2(U), *p2(a[0:2]), *p2(a[2:4]), B, S, 128, _stream()) == 0
    dh = [dout * h[1], dout * h[0]]
    b = [torch.full((R_, 384), float("nan"), device="cuda") for _ in range(4)]
    assert lib.seld_rnn_gru_bwd(*p2(dh), *p2(h), *p2(sv), *p2(U), *p2(b[0:2]), *p2(b[2:4]), B, S, 128, _stream()) == 0
    torch.cuda.synchronize()
    for name, x, y in zip(("dgx_f", "dgx_b", "dgh_f", "dgh_b"), a, b):
        assert bool(torch.isfinite(x).all()) and torch.equal(x, y), name


# ---------------------------------------------------------------- the block and the stage
@pytest.mark.parametrize("name", sorted(R.STAGE_CASES))
def test_rnn_block_and_stage(name):
    """forward in training and in inference (the same function: nothing here depends on the mode but what is saved), the input's and every variable's
    gradient"""
    from seld_amd import modules
    B, S, D, depth, cfg = R.STAGE_CASES[name]
    ref = R.stage_reference(B, S, D, depth, cfg, seed=3)
    tr = ref["specs"]
    stage = (modules.RNN_block if depth is None else modules.RNN_stage)(cfg)((B, S, D))
    rt = stage.blocks[0].rt
    rt.finalize()
    assert [(n, s) for n, _, s in rt.variables] == tr and not rt.state_variables
    assert stage.out_dim == R.out_dim(cfg) and len(stage.blocks) == (depth or 1)
    rt.params[:rt.n_params].copy_(torch.as_tensor(ref["w"]))
    xd = dev(ref["x"].reshape(B * S, D))
    x0 = xd.clone()
    out_eval = stage.forward(xd, B, False).cpu().numpy().copy()
    out = stage.forward(xd, B, True).cpu().numpy().copy()
    dx = stage.backward(dev(ref["dy"].reshape(B * S, -1)), B).cpu().numpy().copy()
    grads = rt.grads[:rt.n_params].cpu().numpy().copy()
    assert torch.equal(xd, x0)
    tag = f"RNN {name}"
    check(f"{tag} forward (training)", out, ref["out"].reshape(B * S, -1))
    check(f"{tag} forward (inference)", out_eval, ref["out"].reshape(B * S, -1))
    check(f"{tag} input gradient", dx, ref["dx"].reshape(B * S, D))
    off, biggest = 0, float(np.abs(ref["grad"]).max())
    for n, s in tr:
        kk = int(np.prod(s))
        _check_or_zero(f"{tag} grad {n}", grads[off:off + kk], ref["grad"][off:off + kk], biggest)
        off += kk


# ---------------------------------------------------------------- the model
def test_train_step_with_an_rnn_stage(seldnet_config):
    """models.seldnet with a small mother_block FIRST and SECOND = RNN_stage (LSTM, concat, depth 2: the heads read 256 features): variable list,
    outputs, both losses and every gradient of one train step at B = 2; then a ragged batch of 1 and a test_step on the same model"""
    from oracle import seldnet_oracle as O
    from seld_amd import losses, models, train
    from test_modules_gpu import STAGE_FIRST
    cfg = R.model_case(seldnet_config, STAGE_FIRST)
    B, T_ = R.MODEL_INPUT[:2]
    tr, nt = R.variable_specs(cfg, R.MODEL_INPUT)
    w, st = R.random_weights(cfg, R.MODEL_INPUT, seed=11)
    x, ys, yd = O.synthetic_batch(B, T_, seed=23)
    model = models.seldnet(R.MODEL_INPUT, cfg)
    assert type(model).__name__ == "ComposedSeldNet"
    assert [(n, s) for n, _, s in model.variables] == tr and [(n, s) for n, _, s in model.state_variables] == nt
    assert ("rnn1.bwd.kernel", (256, 512)) in tr and ("sed.dense0.kernel", (1, 256, 128)) in tr and not any(n.startswith("gru") for n, _ in tr)
    w0, _ = model.get_weights()      # the initial values: orthogonal recurrent kernels, unit forget bias
    d0 = {n: w0[o:o + int(np.prod(s))].reshape(s) for n, o, s in model.variables}
    Uk = d0["rnn0.fwd.recurrent_kernel"].astype(np.float64)
    assert np.abs(Uk @ Uk.T - np.eye(128)).max() < 1e-5
    assert np.array_equal(d0["rnn0.fwd.bias"], np.repeat([0, 1, 0, 0], 128).astype(np.float32))
    model.set_weights(w, st)
    ref = R.train_step(cfg, R.MODEL_INPUT, w, st, x, ys, yd, doa_loss="MSE", loss_weight=(1.0, 1000.0), lr=1e-3, step=1)
    cfg_eval = R.test_step(cfg, R.MODEL_INPUT, w, st, x[:1], ys[:1], yd[:1])
    lw = (1.0, 1000.0)
    # the inference-side checks run first: the train step below moves the weights
    y1, sl1, dl1 = train.teststep(model, x[:1], (ys[:1], yd[:1]), losses.BinaryCrossentropy(), losses.get_doa_loss("MSE"))
    inf = model(x[:1], training=False)
    for k, got in (("sed", y1[0]), ("doa", y1[1]), ("sloss", sl1), ("dloss", dl1)):
        check(f"rnn model ragged test_step {k}", got.cpu().numpy(), cfg_eval[k])
    assert torch.equal(inf[0], y1[0]) and torch.equal(inf[1], y1[1]), "test_step and inference differ"
    y_p, sl, dl = train.trainstep(model, x, (ys, yd), losses.BinaryCrossentropy(), losses.get_doa_loss("MSE"), lw, train.Adam(1e-3))
    check("rnn model trainstep sed", y_p[0].cpu().numpy(), ref["sed"])
    check("rnn model trainstep doa", y_p[1].cpu().numpy(), ref["doa"])
    check("rnn model sloss", sl.cpu().numpy(), ref["sloss"])
    check("rnn model dloss", dl.cpu().numpy(), ref["dloss"])
    g = model.get_grads()
    biggest = np.abs(ref["grad"]).max()
    for n, off, sh in model.variables:
        k = int(np.prod(sh))
        _check_or_zero(f"rnn model grad {n}", g[off:off + k], ref["grad"][off:off + k], biggest)
    # a ragged batch of 1 trains on the same model (buffers sized for 2)
    model.set_weights(w, st)
    ref1 = R.train_step(cfg, R.MODEL_INPUT, w, st, x[:1], ys[:1], yd[:1], doa_loss="MSE", loss_weight=lw, lr=1e-3, step=1)
    y_q, _, _ = train.trainstep(model, x[:1], (ys[:1], yd[:1]), losses.BinaryCrossentropy(), losses.get_doa_loss("MSE"), lw, train.Adam(1e-3))
    check("rnn model ragged trainstep sed", y_q[0].cpu().numpy(), ref1["sed"])
    g1 = model.get_grads()
    for n, off, sh in model.variables:
        k = int(np.prod(sh))
        _check_or_zero(f"rnn model ragged grad {n}", g1[off:off + k], ref1["grad"][off:off + k], np.abs(ref1["grad"]).max())
