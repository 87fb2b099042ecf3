"""The any-width GRU recurrence on the device: seld_rnn_gruw_fwd / _bwd (seld_amd/csrc/gru_w.hip) against rnn_oracle's fp64 step loops at the
project's bar (helpers.check: max|d| / max|ref| <= 1e-4, per direction, dgx / dgh per gate third, saved per plane) over the widths, lengths
and batches tests/gru_width_cases.py derives from seld_rnn_gruw_plan; then the blocks and models that route to it (modules' any_units,
ConvTemporalNet search=True) and the search's main on a tiny data set.

Every operand of a kernel call sits inside a NaN-filled allocation (test_attention_gpu._Window) with an ODD band of floats in front and
behind — no pointer is aligned beyond 4 bytes — and after the call every float outside the [B,S,.] windows still holds the sentinel's bits
and every input holds the bits it had."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import conv_temporal_oracle as CT
import gru_width_cases as G
import rnn_oracle as R
from helpers import check, dev
from test_attention_gpu import _Window, _check_or_zero, _stream

pytestmark = pytest.mark.gpu

BAND = 1025
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)


def _win(rows, cols, data=None):
    return _Window(rows, cols, None, None, BAND, BAND, data)


def _pair(ws, nd):
    return (ws[0].ptr(), ws[1].ptr() if nd == 2 else None)


def _forward(lib, ins, B, S, u, nd=2, save=True, entry="seld_rnn_gruw_fwd"):
    """-> (h windows, saved windows or None)"""
    gx = [_win(B * S, 3 * u, ins["gx"][d]) for d in range(nd)]
    U = [_win(u, 3 * u, ins["U"][d]) for d in range(nd)]
    br = [_win(1, 3 * u, ins["brec"][d]) for d in range(nd)]
    h = [_win(B * S, u) for _ in range(nd)]
    sv = [_win(B * S, 4 * u) for _ in range(nd)] if save else None
    for t in gx + U + br:
        t.snapshot()
    svp = _pair(sv, nd) if save else (None, None)
    assert getattr(lib, entry)(*_pair(gx, nd), *_pair(U, nd), *_pair(br, nd), *_pair(h, nd), *svp, B, S, u, _stream()) == 0
    torch.cuda.synchronize()
    for t in gx + U + br:
        t.assert_unchanged("a forward input")
    for t in h + (sv or []):
        t.assert_band("a forward output")
    return h, sv


def _backward(lib, ins, B, S, u, h, sv, nd=2, entry="seld_rnn_gruw_bwd"):
    """h, sv: windows (the kernel's own forward) or numpy per direction (the oracle's) -> (dgx, dgh) numpy per direction"""
    h = [t if isinstance(t, _Window) else _win(B * S, u, t) for t in h]
    sv = [t if isinstance(t, _Window) else _win(B * S, 4 * u, t) for t in sv]
    dh = [_win(B * S, u, ins["dh"][d]) for d in range(nd)]
    U = [_win(u, 3 * u, ins["U"][d]) for d in range(nd)]
    dgx, dgh = [_win(B * S, 3 * u) for _ in range(nd)], [_win(B * S, 3 * u) for _ in range(nd)]
    for t in dh + U + h + sv:
        t.snapshot()
    assert getattr(lib, entry)(*_pair(dh, nd), *_pair(h, nd), *_pair(sv, nd), *_pair(U, nd), *_pair(dgx, nd), *_pair(dgh, nd), B, S, u, _stream()) == 0
    torch.cuda.synchronize()
    for t in dh + U + h + sv:
        t.assert_unchanged("a backward input")
    for t in dgx + dgh:
        t.assert_band("a backward output")
    return [t.numpy().reshape(B, S, 3 * u) for t in dgx], [t.numpy().reshape(B, S, 3 * u) for t in dgh]


def _run(lib, ins, B, S, u, nd=2):
    """training forward, BPTT from it -> {h, saved, dgx, dgh} per direction"""
    h, sv = _forward(lib, ins, B, S, u, nd)
    dgx, dgh = _backward(lib, ins, B, S, u, h, sv, nd)
    return {"h": [t.numpy().reshape(B, S, u) for t in h], "saved": [t.numpy().reshape(B, S, u, 4) for t in sv], "dgx": dgx, "dgh": dgh}


def _first(ref):
    return {k: v[:1] for k, v in ref.items()}


def _case(lib, B, S, u, scale=1.0):
    ins, ref = G.reference(B, S, u, scale)
    tag = f"gruw u{u} B{B} S{S}" + (f" x{scale}" if scale != 1.0 else "")
    got = _run(lib, ins, B, S, u)
    G.compare(tag, got, ref, u, 1e-4)
    # inference: saved NULL, the training forward's bits
    h0, _ = _forward(lib, ins, B, S, u, save=False)
    for d in (0, 1):
        assert np.array_equal(bits(h0[d].numpy().reshape(B, S, u)), bits(got["h"][d])), f"{tag}: h[{d}] differs without saved"
    # BPTT alone, on the oracle's forward values
    dgx, dgh = _backward(lib, ins, B, S, u, [R.f32(a) for a in ref["h"]], [R.f32(R.gru_saved(ref, d)) for d in (0, 1)])
    G.compare(f"{tag} bptt alone", {"dgx": dgx, "dgh": dgh}, ref, u, 1e-4)
    # one direction
    one = _run(lib, ins, B, S, u, nd=1)
    G.compare(f"{tag} one direction", one, _first(ref), u, 1e-4)


@pytest.mark.parametrize("u", G.widths())
def test_kernel_parity_over_lengths_and_batches(seld_lib, u):
    for B, S in G.cases(u):
        _case(seld_lib, B, S, u)


@pytest.mark.parametrize("form,u", sorted(G.one_width_per_form().items()))
def test_saturated_gates(seld_lib, form, u):
    B, S, scale = G.SATURATED
    _case(seld_lib, B, S, u, scale)


@pytest.mark.parametrize("u", [3, 255] + sorted(G.one_width_per_form().values()))
def test_two_calls_give_the_same_bits_and_a_clip_does_not_depend_on_its_batch(seld_lib, u):
    t = G.gruw_plan(u)[0][1]
    B, S = t + 1, 9
    ins, _ = G.reference(B, S, u)
    a, b = _run(seld_lib, ins, B, S, u), _run(seld_lib, ins, B, S, u)
    for k in a:
        for d in (0, 1):
            assert np.array_equal(bits(a[k][d]), bits(b[k][d])), f"u{u} {k}[{d}]: two calls differ"
    for clip in sorted({0, 1, t - 1, t}):
        alone = {k: (v[:, clip:clip + 1] if k in ("gx", "dh") else v) for k, v in ins.items()}
        c = _run(seld_lib, alone, 1, S, u)
        for k in a:
            for d in (0, 1):
                assert np.array_equal(bits(c[k][d][0]), bits(a[k][d][clip])), f"u{u} {k}[{d}]: clip {clip} of {B} differs from that clip alone"


def test_at_128_both_entries_meet_the_bar(seld_lib):
    B, S, u = 3, 17, 128
    ins, ref = G.reference(B, S, u)
    G.compare("gruw at 128", _run(seld_lib, ins, B, S, u), ref, u, 1e-4)
    h, sv = _forward(seld_lib, ins, B, S, u, entry="seld_rnn_gru_fwd")
    dgx, dgh = _backward(seld_lib, ins, B, S, u, h, sv, entry="seld_rnn_gru_bwd")
    got = {"h": [t.numpy().reshape(B, S, u) for t in h], "saved": [t.numpy().reshape(B, S, u, 4) for t in sv], "dgx": dgx, "dgh": dgh}
    G.compare("seld_rnn_gru_* at 128", got, ref, u, 1e-4)


# ---------------------------------------------------------------- blocks through seld_amd.modules
def _stage_check(tag, stage, ref, B, S, D):
    rt = stage.blocks[0].rt
    rt.finalize()
    tr = ref["specs"]
    assert [(n, s) for n, _, s in rt.variables] == tr and not rt.state_variables
    rt.params[:rt.n_params].copy_(torch.as_tensor(ref["w"]))
    xd = dev(ref["x"].reshape(B * S, D))
    x0 = xd.clone()
    out_eval = stage.forward(xd, B, False).cpu().numpy().copy()
    out = stage.forward(xd, B, True).cpu().numpy().copy()
    dx = stage.backward(dev(ref["dy"].reshape(B * S, -1)), B).cpu().numpy().copy()
    grads = rt.grads[:rt.n_params].cpu().numpy().copy()
    assert torch.equal(xd, x0)
    check(f"{tag} forward (training)", out, ref["out"].reshape(B * S, -1))
    check(f"{tag} forward (inference)", out_eval, ref["out"].reshape(B * S, -1))
    check(f"{tag} input gradient", dx, ref["dx"].reshape(B * S, D))
    off, biggest = 0, float(np.abs(ref["grad"]).max())
    for n, s in tr:
        kk = int(np.prod(s))
        _check_or_zero(f"{tag} grad {n}", grads[off:off + kk], ref["grad"][off:off + kk], biggest)
        off += kk


def _any_units_rt():
    from seld_amd import modules
    rt = modules._Rt(torch.device("cuda", torch.cuda.current_device()))
    rt.any_units = True
    return rt


@pytest.mark.parametrize("name", sorted(G.BLOCK_CASES))
def test_rnn_block_at_24_units(name):
    from seld_amd import modules
    kind, B, S, D, depth, cfg = G.BLOCK_CASES[name]
    ref = R.stage_reference(B, S, D, depth, cfg, seed=3)
    stage = modules._build_second(kind, _any_units_rt(), cfg, S, D, B, prefix="rnn")
    assert stage.out_dim == R.out_dim(cfg) and stage.blocks[0].u == 24
    _stage_check(name, stage, ref, B, S, D)


def test_bidirectional_gru_block_with_a_width_per_layer():
    from seld_amd import modules
    B, S, D, cfg = G.GRU_BLOCK_CASE
    ref = G.gru_block_reference(B, S, D, cfg, seed=3)
    stage = modules._build_second("bidirectional_GRU_block", _any_units_rt(), cfg, S, D, B, prefix="gru")
    assert [blk.u for blk in stage.blocks] == cfg["units"] and stage.out_dim == cfg["units"][-1]
    _stage_check("bidirectional_GRU_block [12, 128, 5]", stage, ref, B, S, D)


# ---------------------------------------------------------------- models
@pytest.mark.parametrize("name", sorted(G.MODELS))
def test_model_against_the_oracle(name):
    """inference, a training forward, one train step (outputs, both losses, the flat gradient, every variable's gradient, the
    BatchNormalization state) and a batch smaller than the built one"""
    from seld_amd import losses, models, train
    cfg, shape, w, st, x, ys, yd, ref = G.model_reference(name)
    tr, nt = CT.variable_specs(cfg, shape)
    model = models.conv_temporal(shape, cfg, search=True)
    assert [(n, s) for n, _, s in model.variables] == tr and [(n, s) for n, _, s in model.state_variables] == nt
    model.set_weights(w, st)
    tag = f"conv_temporal search {name}"
    y_i = model(x, training=False)
    check(f"{tag} inference sed", y_i[0].cpu().numpy(), ref["infer"][0])
    check(f"{tag} inference doa", y_i[1].cpu().numpy(), ref["infer"][1])
    y_p, sl, dl = train.trainstep(model, x, (ys, yd), losses.BinaryCrossentropy(), losses.MSE, (1.0, 1000.0), train.Adam(1e-3))
    check(f"{tag} trainstep sed", y_p[0].cpu().numpy(), ref["sed"])
    check(f"{tag} trainstep doa", y_p[1].cpu().numpy(), ref["doa"])
    check(f"{tag} sloss", sl.cpu().numpy(), ref["sloss"])
    check(f"{tag} dloss", dl.cpu().numpy(), ref["dloss"])
    g = model.get_grads()
    check(f"{tag} flat gradient", g, ref["grad"])
    biggest = np.abs(ref["grad"]).max()
    for n, off, sh in model.variables:
        k = int(np.prod(sh))
        _check_or_zero(f"{tag} grad {n}", g[off:off + k], ref["grad"][off:off + k], biggest)
    w1, st1 = model.get_weights()
    check(f"{tag} BN state", st1, ref["new_state"])
    nb = shape[0] - 1
    y2 = model(x[:nb], training=False)
    sed2, doa2 = CT.inference(cfg, shape, w1, st1, x[:nb])
    assert tuple(y2[0].shape) == (nb,) + ref["sed"].shape[1:]
    check(f"{tag} batch of {nb} sed", y2[0].cpu().numpy(), sed2)
    check(f"{tag} batch of {nb} doa", y2[1].cpu().numpy(), doa2)
    y3, _, _ = train.trainstep(model, x[:nb], (ys[:nb], yd[:nb]), losses.BinaryCrossentropy(), losses.MSE, (1.0, 1000.0), train.Adam(1e-3))
    assert tuple(y3[1].shape) == (nb,) + ref["doa"].shape[1:] and bool(torch.isfinite(y3[0]).all()) and np.isfinite(model.get_grads()).all()
    model.close()


def _one_step(cfg, shape, search, training_only=False):
    from seld_amd import losses, models, train
    w, st = CT.random_weights(cfg, shape, seed=11)
    x, ys, yd = CT.synthetic_batch(cfg, shape, seed=23)
    model = models.conv_temporal(shape, cfg, search=search)
    model.set_weights(w, st)
    y_p, sl, dl = train.trainstep(model, x, (ys, yd), losses.BinaryCrossentropy(), losses.MSE, (1.0, 1000.0), train.Adam(1e-3))
    out = [y_p[0].cpu().numpy(), y_p[1].cpu().numpy(), sl.cpu().numpy(), dl.cpu().numpy(), model.get_grads(), *model.get_weights()]
    model.close()
    return out


def test_search_changes_nothing_at_128_units():
    """SS5's small chain (128-unit GRU head, every Dropout at 0) built with search=True and search=False: the same bits"""
    a, b = _one_step(CT.SS5_SMALL, CT.SS5_SMALL_INPUT, True), _one_step(CT.SS5_SMALL, CT.SS5_SMALL_INPUT, False)
    for i, (p, q) in enumerate(zip(a, b)):
        assert np.array_equal(bits(p), bits(q)), f"quantity {i} differs"


DENSE_CFG = {
    "n_classes": 3, "filters": 4, "first_kernel_size": 3, "first_pool_size": [2, 2],
    "BLOCK0": "simple_dense_stage", "BLOCK0_ARGS": {"depth": 1, "units": 64, "dense_activation": "relu", "dropout_rate": 0.5},
    "SED": "simple_dense_stage", "SED_ARGS": {"depth": 1, "units": 8, "dense_activation": "relu", "dropout_rate": 0},
    "DOA": "simple_dense_stage", "DOA_ARGS": {"depth": 1, "units": 8, "dense_activation": "relu", "dropout_rate": 0},
}
DENSE_INPUT = (4, 20, 8, 3)


def test_dense_dropout_under_search():
    from seld_amd import models
    with pytest.raises(ValueError, match="dropout_rate must be 0"):
        models.conv_temporal(DENSE_INPUT, DENSE_CFG, "meta")
    w, st = CT.random_weights(DENSE_CFG, DENSE_INPUT, seed=11)
    x, _, _ = CT.synthetic_batch(DENSE_CFG, DENSE_INPUT, seed=23)
    model = models.conv_temporal(DENSE_INPUT, DENSE_CFG, search=True)
    model.set_weights(w, st)
    y = model.body[0].layers[0][1]      # the dense layer's output behind its activation and Dropout
    lin = model.body[0].layers[0][0]
    model(x, training=False)
    live = (lin.z[:y.shape[0]] != 0)      # the stage's activation is None (canonical_kind): a pre-activation is never exactly 0
    assert bool(live.all()) and bool((y != 0).all()), "inference dropped something"
    kept_eval = y.clone()
    model(x, training=True)
    frac = float((y == 0).float().mean())
    assert 0.4 < frac < 0.6, f"rate 0.5 zeroed {frac:.3f} of the units"
    model.set_weights(w, st)      # the training forward moved the stem's BatchNormalization statistics
    model(x, training=False)
    assert torch.equal(y, kept_eval)
    model.close()
    zero = copy.deepcopy(DENSE_CFG)
    zero["BLOCK0_ARGS"]["dropout_rate"] = 0
    a, b = _one_step(zero, DENSE_INPUT, True), _one_step(zero, DENSE_INPUT, False)
    for i, (p, q) in enumerate(zip(a, b)):
        assert np.array_equal(bits(p), bits(q)), f"rate 0: quantity {i} differs from search=False"


# ---------------------------------------------------------------- the search's main
def test_nas_seldnet_main_on_a_tiny_dataset(tmp_path, monkeypatch):
    from seld_amd import nas_seldnet as N
    nc, F, Cc, win, fpl = 3, 8, 7, 4, 5      # input [20, 8, 7]: 4 labels of 5 frames
    rng = np.random.default_rng(5)
    for d in ("foa_dev_norm", "foa_dev_label"):
        os.makedirs(tmp_path / d)
    for fold in (1, 2, 6):
        L = 2 * win
        np.save(tmp_path / "foa_dev_norm" / f"fold{fold}_a.npy", R.f32(rng.standard_normal((L * fpl, F, Cc))))
        sed = (rng.random((L, nc)) < 0.3).astype(np.float32)
        doa = R.f32(rng.uniform(-1, 1, (L, 3 * nc))) * np.tile(sed, 3)
        np.save(tmp_path / "foa_dev_label" / f"fold{fold}_a.npy", np.concatenate([sed, doa], -1))
    monkeypatch.setattr(N, "search_space_2d", {"mother_stage": {
        "depth": [1], "filters0": [0], "filters1": [4, 6], "filters2": [0], "kernel_size0": [1], "kernel_size1": [1, 3], "kernel_size2": [1],
        "connect0": [[0], [1]], "connect1": [[0, 0], [1, 0]], "connect2": [[0, 0, 0], [1, 0, 1]], "strides": [(1, 2)]}})
    monkeypatch.setattr(N, "search_space_1d", {
        "bidirectional_GRU_stage": {"depth": [1, 2], "units": [4, 12]},
        "simple_dense_stage": {"depth": [1], "units": [4, 8], "dense_activation": ["relu"], "dropout_rate": [0., 0.5]}})
    name = str(tmp_path / "run")
    argv = ["--name", name, "--dataset_path", str(tmp_path), "--n_samples", "3", "--n_blocks", "2", "--min_flops", "0", "--max_flops", "0",
            "--batch_size", "2", "--n_repeat", "2", "--n_classes", str(nc), "--label_window_size", str(win), "--time_mask_size", "4",
            "--freq_mask_size", "3"]
    real, calls = N.train_and_eval, []

    def interrupted(*a, **kw):      # the run is cut off in its third sample
        if len(calls) == 2:
            raise KeyboardInterrupt
        calls.append(1)
        return real(*a, **kw)
    monkeypatch.setattr(N, "train_and_eval", interrupted)
    with pytest.raises(KeyboardInterrupt):
        N.main(argv)
    monkeypatch.setattr(N, "train_and_eval", real)
    with open(name + ".json") as f:
        first = json.load(f)
    assert sorted(k for k in first if k.isdigit()) == ["000", "001"]
    keys = {"loss", "val_loss", "test_error_rate", "test_f1score", "test_der", "test_derf", "test_seld_score", "flops", "params", "time"}
    widths = set()
    for k in ("000", "001"):
        perf, cfg = first[k]["perf"], first[k]["config"]
        assert set(perf) == keys, set(perf) ^ keys
        assert all(np.isfinite(np.asarray(v, np.float64)).all() for v in perf.values()), perf
        assert cfg["SED"] in N.search_space_1d and cfg["DOA"] in N.search_space_1d and cfg["n_classes"] == nc
        widths |= {a["units"] for kk, a in cfg.items() if kk.endswith("_ARGS") and "units" in a}
    assert widths <= {4, 8, 12}
    second = N.main(argv)      # resumes at sample 2
    assert sorted(k for k in second if k.isdigit()) == ["000", "001", "002"]
    assert second["000"] == first["000"] and second["001"] == first["001"]
    with open(name + ".json") as f:
        assert json.load(f) == json.loads(json.dumps(second))
    kinds = [second[k]["config"][b] for k in ("000", "001", "002") for b in ("BLOCK0", "BLOCK1", "SED", "DOA")]
    assert "bidirectional_GRU_stage" in kinds, "the seeded draws hold no GRU stage: the run did not reach seld_rnn_gruw_*"
