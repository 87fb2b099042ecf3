"""The voice-activity model on the device: the seld_vad_* operators (seld_amd/csrc/vad.hip) one by one through the C ABI, then
models.spectro_temporal_attention_based_VAD (seld_amd/vad.py) against the fp64 restatement tests/vad_oracle.py at the project's bar
(helpers.check: max|d| / max|ref| <= 1e-4).  tests/test_vad_cpu.py asserts, on the same cases, that plain fp32 stays within 5e-5 of fp64 and
that the model cases whose gradients are compared keep their decision margins.

Outputs are written into NaN-filled allocations with a band behind them that must still be NaN after the call.  Gradients that are zero by
mathematics (a bias in front of training-mode BatchNormalization) are asserted absolutely: |g| <= 1e-4 max|the layer's kernel gradient|.

Default-shape gradients are NOT compared: with 4 x 7 x 40 x 16 pooled pairs in the first stage alone the smallest pair gap is ~ 6e-6 of the
tensor's maximum, below fp32's own error, and a flipped pair moves one pixel's gradient whole."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import vad_oracle as V
from helpers import REL_TOL, check, dev, ptr
from test_vad_cpu import refusal_checks

pytestmark = pytest.mark.gpu

GUARD = 257
bits = lambda t: t.contiguous().view(torch.int32)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class _Out:
    """n output elements of `dtype` in front of a sentinel band"""

    def __init__(self, n, dtype=torch.float32):
        self.n = int(n)
        fill = float("nan") if dtype == torch.float32 else 0xAB
        self.buf = torch.full((self.n + GUARD,), fill, dtype=dtype, device="cuda")
        self.guard = self.buf[self.n:].clone()

    def ptr(self):
        return C.c_void_p(self.buf.data_ptr())

    def get(self, *shape):
        g = self.buf[self.n:]
        same = torch.equal(g.view(torch.int32), self.guard.view(torch.int32)) if g.dtype == torch.float32 else torch.equal(g, self.guard)
        assert same, "a value behind the output was written"
        return self.buf[:self.n].reshape(*shape)


# ---------------------------------------------------------------- gate-pool
def _gate_run(lib, a, b, dy, rows, W, Cc, halves=False, idx=True):
    """-> (y, idx, da, db) device tensors; halves: a and b are the column halves of one [rows * W, 2 C + 4] buffer (ld > C), and so are da, db"""
    Wo = W // 2
    if halves:
        ld = 2 * Cc + 4
        buf = torch.full((rows * W, ld), float("nan"), device="cuda")
        gbuf = torch.full((rows * W, ld), float("nan"), device="cuda")
        va, vb, ga, gb = buf[:, :Cc], buf[:, Cc:2 * Cc], gbuf[:, :Cc], gbuf[:, Cc:2 * Cc]
        va.copy_(dev(a.reshape(-1, Cc)))
        vb.copy_(dev(b.reshape(-1, Cc)))
    else:
        ld = Cc
        va, vb = dev(a), dev(b)
        oa, ob = _Out(rows * W * Cc), _Out(rows * W * Cc)
    y, ix = _Out(rows * Wo * Cc), _Out(rows * Wo * Cc, torch.uint8)
    assert lib.seld_vad_gate_pool_fwd(ptr(va), ptr(vb), ld, y.ptr(), ix.ptr() if idx else None, rows, W, Cc, _stream()) == 0
    if not idx:
        torch.cuda.synchronize()
        return y.get(rows, Wo, Cc), None, None, None
    gdy = dev(dy)
    pa, pb = (ptr(ga), ptr(gb)) if halves else (oa.ptr(), ob.ptr())
    assert lib.seld_vad_gate_pool_bwd(ptr(va), ptr(vb), ld, ix.ptr(), ptr(gdy), pa, pb, rows, W, Cc, _stream()) == 0
    torch.cuda.synchronize()
    if halves:
        assert bool(torch.isnan(gbuf[:, 2 * Cc:]).all()) and bool(torch.isnan(buf[:, 2 * Cc:]).all())      # the columns behind the halves
        da, db = ga.contiguous().reshape(rows, W, Cc), gb.contiguous().reshape(rows, W, Cc)
    else:
        da, db = oa.get(rows, W, Cc), ob.get(rows, W, Cc)
    return y.get(rows, Wo, Cc), ix.get(rows, Wo, Cc), da, db


@pytest.mark.parametrize("rows,W,Cc", V.GATE_CASES, ids=lambda v: str(v))
def test_gate_pool_forward_and_backward(seld_lib, rows, W, Cc):
    a, b, dy = V.gate_inputs(rows, W, Cc)
    ry, rwin, rda, rdb = V.gate_reference(a, b, dy)
    y, ix, da, db = _gate_run(seld_lib, a, b, dy, rows, W, Cc)
    check(f"gate {(rows, W, Cc)} y", y.cpu().numpy(), ry)
    assert np.array_equal(ix.cpu().numpy(), rwin)      # gate_inputs keeps every pair 1e-3 apart
    check(f"gate {(rows, W, Cc)} da", da.cpu().numpy(), rda)
    check(f"gate {(rows, W, Cc)} db", db.cpu().numpy(), rdb)
    # losers and the dropped odd column: exactly 0
    Wo = W // 2
    lose = np.stack([rwin == 1, rwin == 0], axis=2).reshape(rows, 2 * Wo, Cc)
    for g in (da.cpu().numpy(), db.cpu().numpy()):
        assert not g[:, :2 * Wo][lose].any() and not g[:, 2 * Wo:].any()
    # inference (no idx): the same bits; a second run: the same bits
    y0 = _gate_run(seld_lib, a, b, dy, rows, W, Cc, idx=False)[0]
    assert torch.equal(bits(y0), bits(y))
    again = _gate_run(seld_lib, a, b, dy, rows, W, Cc)
    for t0, t1 in zip((y, da, db), (again[0], again[2], again[3])):
        assert torch.equal(bits(t0), bits(t1))
    assert torch.equal(ix, again[1])


@pytest.mark.parametrize("rows,W,Cc", [(7, 10, 4), (5, 5, 3), (33, 6, 128)], ids=lambda v: str(v))
def test_gate_pool_on_the_two_halves_of_one_buffer(seld_lib, rows, W, Cc):
    """ld = 2 C + 4 > C: vector path (C % 4 == 0) and scalar path; the same bits as the contiguous call"""
    a, b, dy = V.gate_inputs(rows, W, Cc)
    want = _gate_run(seld_lib, a, b, dy, rows, W, Cc)
    got = _gate_run(seld_lib, a, b, dy, rows, W, Cc, halves=True)
    for t0, t1 in zip((want[0], want[2], want[3]), (got[0], got[2], got[3])):
        assert torch.equal(bits(t0), bits(t1))
    assert torch.equal(want[1], got[1])


def test_gate_pool_ties_resolve_as_pool2d(seld_lib):
    """equal values in a pair: the first stays, as seld_pool2d_fwd records it"""
    rows, W, Cc = 2, 4, 4
    a = np.ones((rows, W, Cc), np.float32)
    b = np.zeros((rows, W, Cc), np.float32)
    y, ix, da, db = _gate_run(seld_lib, a, b, np.ones((rows, 2, Cc), np.float32), rows, W, Cc)
    g = dev(a * 0.5)
    py, pix = _Out(rows * 2 * Cc), _Out(rows * 2 * Cc, torch.uint8)
    assert seld_lib.seld_pool2d_fwd(ptr(g), py.ptr(), pix.ptr(), 1, rows, W, Cc, 1, 2, 0, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(ix.reshape(-1), pix.get(-1)) and not ix.any() and torch.equal(y.reshape(-1), py.get(-1))
    assert torch.equal(da[:, 0::2], torch.full_like(da[:, 0::2], 0.5)) and not da[:, 1::2].any()


# ---------------------------------------------------------------- temporal attention
def _tattn_run(lib, ins, B, T, Nt, H, save=True):
    q, k, v, dy, dscore = (dev(z) for z in ins)
    y, score, P = _Out(B * T * Nt), _Out(B * T), _Out(B * T * H)
    assert lib.seld_vad_tattn_fwd(ptr(q), ptr(k), ptr(v), y.ptr(), score.ptr(), P.ptr() if save else None, B, T, Nt, H, _stream()) == 0
    if not save:
        torch.cuda.synchronize()
        return {"y": y.get(B, T, Nt), "score": score.get(B, T)}
    dq, dk, dv = _Out(B * Nt), _Out(B * T * Nt), _Out(B * T * Nt)
    assert lib.seld_vad_tattn_bwd(ptr(q), ptr(k), ptr(v), P.ptr(), score.ptr(), ptr(dy), ptr(dscore), dq.ptr(), dk.ptr(), dv.ptr(), B, T, Nt, H,
                                  _stream()) == 0
    torch.cuda.synchronize()
    return {"y": y.get(B, T, Nt), "score": score.get(B, T), "P": P.get(B, T, H), "dq": dq.get(B, Nt), "dk": dk.get(B, T, Nt), "dv": dv.get(B, T, Nt)}


@pytest.mark.parametrize("case", V.TATTN_CASES, ids=lambda v: "x".join(map(str, v)))
def test_temporal_attention_forward_and_backward(seld_lib, case):
    """the last case sits on every stated limit at once: T = SELD_VAD_MAX_T, Nt = H = SELD_VAD_MAX_NT (the largest LDS footprint)"""
    B, T, Nt, H = case
    ins = V.tattn_inputs(B, T, Nt, H)
    ref = V.tattn_reference(*ins, H)
    got = _tattn_run(seld_lib, ins, B, T, Nt, H)
    for n in ("y", "score", "P", "dq", "dk", "dv"):
        check(f"tattn {case} {n}", got[n].cpu().numpy(), ref[n])
    inf = _tattn_run(seld_lib, ins, B, T, Nt, H, save=False)
    again = _tattn_run(seld_lib, ins, B, T, Nt, H)
    for n in ("y", "score"):
        assert torch.equal(bits(inf[n]), bits(got[n])), n      # NULL P: the same bits
    for n in got:
        assert torch.equal(bits(again[n]), bits(got[n])), n    # two runs: the same bits


def test_temporal_attention_saturated_keys_stay_finite(seld_lib):
    (B, T, Nt, H), scale = V.TATTN_SATURATED
    ins = V.tattn_inputs(B, T, Nt, H, k_scale=scale)
    assert np.abs(ins[1]).max() > 100
    ref = V.tattn_reference(*ins, H)
    got = _tattn_run(seld_lib, ins, B, T, Nt, H)
    for n in ref:
        check(f"tattn saturated {n}", got[n].cpu().numpy(), ref[n])


def test_refusals_beside_a_live_device(seld_lib):
    """every INVALID / UNSUPPORTED of the eight entries, among them just past each limit of the attention (Nt 516, T 65) whose edges
    test_temporal_attention_forward_and_backward runs; nothing is enqueued and the device stays usable"""
    refusal_checks(seld_lib)
    torch.cuda.synchronize()
    assert float(torch.ones(4, device="cuda").sum()) == 4.0


# ---------------------------------------------------------------- binary cross-entropy
@pytest.mark.parametrize("n", V.BCE_CASES)
def test_bce_loss_gradient_weight_and_accumulate(seld_lib, n):
    p, y = V.bce_inputs(n)
    if n >= 7:
        p[:4], y[:4] = [0.0, 1.0, 0.0, 1.0], [1.0, 0.0, 0.0, 1.0]      # exactly 0 and 1, right and wrong
    else:
        p[0], y[0] = 0.0, 1.0
    t = lambda z: torch.tensor(z, dtype=torch.float64)
    rl, rg = float(V.bce(t(y), t(p))), V.bce_grad(t(y), t(p), 0.75).numpy()
    gp, gy = dev(p), dev(y)
    scratch = torch.full((int(seld_lib.seld_vad_bce_scratch(n)),), float("nan"), device="cuda")
    loss, dp = _Out(1), _Out(n)
    assert seld_lib.seld_vad_bce(ptr(gp), ptr(gy), loss.ptr(), dp.ptr(), ptr(scratch), n, 0.75, 0, _stream()) == 0
    torch.cuda.synchronize()
    l1, g1 = float(loss.get(1)[0]), dp.get(n).cpu().numpy()
    assert np.isfinite(l1) and np.isfinite(g1).all()
    check(f"bce {n} loss", l1, 0.75 * rl)
    check(f"bce {n} dp", g1, rg)
    clipped = (p <= 0) | (p >= 1)
    assert clipped.any() and not g1[clipped].any()      # the clip is active: exactly 0
    # accumulate adds a second output's loss; NULL dp gives the same loss bits
    assert seld_lib.seld_vad_bce(ptr(gp), ptr(gy), loss.ptr(), None, ptr(scratch), n, 0.5, 1, _stream()) == 0
    torch.cuda.synchronize()
    check(f"bce {n} accumulated", float(loss.get(1)[0]), 1.25 * rl)
    l2 = _Out(1)
    assert seld_lib.seld_vad_bce(ptr(gp), ptr(gy), l2.ptr(), None, ptr(scratch), n, 0.75, 0, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(bits(l2.get(1)), bits(torch.tensor([l1], device="cuda")))


# ---------------------------------------------------------------- windows
@pytest.mark.parametrize("window,L,D", [(V.REF_WINDOW, 60, 80), (V.REF_WINDOW, 39, 1), ([0], 5, 1), ([0, 2, 3], 9, 80)], ids=lambda v: str(v)[:12])
def test_windows_and_unwindow(seld_lib, window, L, D):
    """the reference's table, len = max(offs) + 1 (one window), a single-offset table; D = 1 and 80"""
    from seld_amd import vad
    rng = np.random.default_rng(L)
    x = rng.standard_normal((L, D)).astype(np.float32)
    wins = vad.seq_to_windows(dev(x), window)
    torch.cuda.synchronize()
    assert np.array_equal(wins.cpu().numpy(), V.seq_to_windows(x, window))      # values are moved, not computed
    y = rng.standard_normal(wins.shape).astype(np.float32)
    seq = vad.windows_to_seq(dev(y), window)
    assert tuple(seq.shape) == (L, D)
    check(f"unwindow {L}x{D}", seq.cpu().numpy(), V.windows_to_seq(y, window))
    const = vad.windows_to_seq(vad.seq_to_windows(torch.full((L, D), 2.5, device="cuda"), window), window).cpu().numpy()
    n = L - max(window)
    covered = np.array([any(0 <= m - o < n for o in window) for m in range(L)])
    assert np.allclose(const[covered], 2.5, rtol=0, atol=1e-6) and not const[~covered].any()
    # straight through the C ABI with a guarded output
    out = _Out(n * len(window) * D)
    offs = (C.c_int32 * len(window))(*window)
    assert seld_lib.seld_vad_windows(ptr(dev(x)), out.ptr(), offs, len(window), L, D, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(out.get(*wins.shape), wins)


# ---------------------------------------------------------------- the model
def _build(cfg, shape, w, st, dropout=False, **kw):
    from seld_amd import vad
    model = vad.SpectroTemporalVAD(shape, cfg, dropout=dropout, **kw)
    tr, nt = V.variable_specs(cfg, shape)
    assert [(n, sh) for n, _, sh in model.variables] == tr and [(n, sh) for n, _, sh in model.state_variables] == nt
    model.set_weights(w, st)
    return model


def _fwd_bwd(model, x, y, loss_weights=(1.0, 1.0, 1.0)):
    """forward, loss and backward without the optimizer -> (outs, loss, grads, state)"""
    xt = model._prep(x)
    outs = model._forward(xt, True)
    loss = model._loss(outs, model._label(y, xt.shape[0]), loss_weights, True)
    model._backward(xt.shape[0])
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs], float(loss), model.get_grads(), model.get_weights()[1]


def _check_grads(tag, cfg, shape, got, ref):
    tr, _ = V.variable_specs(cfg, shape)
    zero, off, by = V.zero_bias_names(cfg, shape), 0, {}
    for n, sh in tr:
        k = int(np.prod(sh))
        by[n] = (got[off:off + k], ref[off:off + k])
        off += k
    for n, (g, r) in by.items():
        if n in zero:      # identically 0 in exact arithmetic: absolute, against the layer's kernel gradient
            assert np.abs(g).max() <= REL_TOL * np.abs(by[zero[n]][1]).max(), f"{tag} {n}"
        else:
            check(f"{tag} grad {n}", g, r)


@functools.lru_cache(maxsize=None)
def _model_reference(name):
    cfg, shape, w, st, x, y, masks = V.model_case(name)
    return V.train_step(cfg, shape, w, st, x, y, masks=masks)


@pytest.mark.parametrize("name", ["even", "odd"])
def test_model_forward_loss_and_every_gradient(name):
    cfg, shape, w, st, x, y, _ = V.model_case(name)
    ref = _model_reference(name)
    model = _build(cfg, shape, w, st)
    outs, loss, grads, state = _fwd_bwd(model, x, y)
    for n, o in zip(("out", "pipe", "score"), outs):
        assert o.shape == ref[n].shape
        check(f"{name} {n}", o, ref[n])
    check(f"{name} loss", loss, ref["loss"])
    check(f"{name} moving statistics", state, ref["state"])
    _check_grads(name, cfg, shape, grads, ref["grad"])


def test_model_fused_and_composed_gate_paths_agree():
    cfg, shape, w, st, x, y, _ = V.model_case("odd")
    runs = [_fwd_bwd(_build(cfg, shape, w, st, fused_gate=f), x, y) for f in (True, False)]
    for a, b in zip(runs[0][0], runs[1][0]):
        check("fused vs composed output", a, b)
    _check_grads("fused vs composed", cfg, shape, runs[0][2], runs[1][2])
    _check_grads("composed", cfg, shape, runs[1][2], _model_reference("odd")["grad"])


def test_model_default_config_forward_loss_and_inference():
    from seld_amd import models
    cfg, shape = V.DEFAULT_CFG, V.DEFAULT_INPUT
    w, st = V.random_weights(cfg, shape, 5)
    x, y = V.case_inputs(shape[0], shape[1:], 5)
    ref = V.train_step(cfg, shape, w, st, x, y)
    model = models.spectro_temporal_attention_based_VAD(shape, cfg)
    assert [(n, sh) for n, _, sh in model.variables] == V.variable_specs({}, shape)[0] and model.n_params == 559298
    model.set_weights(w, st)
    outs, loss = model.test_step(x, y)      # inference: the moving statistics, no state change
    for n, o, r in zip(("out", "pipe", "score"), outs, V.infer(cfg, shape, w, st, x)):
        check(f"default inference {n}", o.cpu().numpy(), r)
    assert np.array_equal(model.get_weights()[1], st)
    assert [tuple(o.shape[1:]) for o in outs] == [(7, 1), (7, 1), (7,)]      # models_test.py:51-53
    outs, loss, _, state = _fwd_bwd(model, x, y)
    for n, o in zip(("out", "pipe", "score"), outs):
        check(f"default {n}", o, ref[n])
    check("default loss", loss, ref["loss"])
    check("default moving statistics", state, ref["state"])
    assert np.allclose(outs[2].sum(axis=1), 1.0, atol=1e-5)
    assert "Trainable params: 559298" in model.summary()


def test_model_dropout_draws_the_library_masks():
    cfg, shape, w, st, x, y, masks = V.model_case("dropout")
    ref = _model_reference("dropout")
    with pytest.raises(ValueError):
        _build(cfg, shape, w, st, dropout=False)      # a rate above 0 needs dropout=True
    model = _build(cfg, shape, w, st, dropout=True)
    assert model.dropout_step == 0
    outs, loss, grads, _ = _fwd_bwd(model, x, y)
    assert model.dropout_step == 1
    for n, o in zip(("out", "pipe", "score"), outs):
        check(f"dropout {n}", o, ref[n])
    check("dropout loss", loss, ref["loss"])
    _check_grads("dropout", cfg, shape, grads, ref["grad"])
    # the next step draws other masks; inference draws none and is repeatable
    model.set_weights(w, st)
    outs2 = _fwd_bwd(model, x, y)[0]
    assert model.dropout_step == 2 and np.abs(outs2[0] - outs[0]).max() > 1e-3
    model.set_weights(w, st)
    a, b = [o.cpu().numpy() for o in model(x)], [o.cpu().numpy() for o in model(x)]
    assert model.dropout_step == 2 and all(np.array_equal(p, q) for p, q in zip(a, b))
    for n, o, r in zip(("out", "pipe", "score"), a, V.infer(cfg, shape, w, st, x)):
        check(f"dropout model inference {n}", o, r)


def test_model_two_adam_steps():
    from seld_amd import train
    cfg, shape, seed, lr = V.ADAM_CASE
    w, st = V.random_weights(cfg, shape, seed)
    batches = [V.case_inputs(shape[0], shape[1:], seed + i) for i in range(2)]
    rw, rst, rlosses = V.adam_steps(cfg, shape, w, st, batches, lr=lr)
    model = _build(cfg, shape, w, st)
    losses = [float(model.train_step(x, y, train.Adam(lr))[1]) for x, y in batches]
    gw, gst = model.get_weights()
    check("adam losses", losses, rlosses)
    check("adam moving statistics", gst, rst)
    assert np.abs(gst - st).max() > 1e-4      # the moving statistics move
    # weights, variable by variable.  A bias in front of a BatchNormalization has a gradient of rounding noise, which Adam normalises to a
    # step of up to lr whatever its size; the model's function does not depend on that bias, so it is held to Adam's bound instead: 2 lr
    tr, _ = V.variable_specs(cfg, shape)
    zero, off = V.zero_bias_names(cfg, shape), 0
    for n, sh in tr:
        k = int(np.prod(sh))
        if n in zero:
            assert np.abs(gw[off:off + k] - w[off:off + k]).max() <= 2 * lr * 1.0001, n
        else:
            check(f"adam {n}", gw[off:off + k], rw[off:off + k])
            assert np.abs(gw[off:off + k] - w[off:off + k]).max() > 0.5 * lr, n      # and it moved
        off += k


def test_model_adabelief_step_runs_on_the_v2_optimizer():
    """train_vad_baseline.py:47: AdaBelief; one step from zero slots against tests/trainv2_oracle.adabelief on the device's own gradient"""
    import trainv2_oracle as T2
    from seld_amd import trainv2
    cfg, shape, w, st, x, y, _ = V.model_case("even")
    model = _build(cfg, shape, w, st)
    model.train_step(x, y, trainv2.AdaBelief(1e-3))
    torch.cuda.synchronize()
    g = torch.tensor(_model_reference("even")["grad"])
    want, _, _ = T2.adabelief(torch.tensor(w, dtype=torch.float64), g, torch.zeros_like(g), torch.zeros_like(g), 1, lr=1e-3)
    tr, _ = V.variable_specs(cfg, shape)
    zero, off, gw = V.zero_bias_names(cfg, shape), 0, model.get_weights()[0]
    for n, sh in tr:
        k = int(np.prod(sh))
        if n not in zero:
            check(f"adabelief {n}", gw[off:off + k], want.numpy()[off:off + k])
        off += k
    model.close()


def test_predict_sequence():
    from seld_amd import vad
    cfg, shape = V.SMALL_CFG, (8, 7, 10, 1)
    w, st = V.random_weights(cfg, shape, 2)
    x = np.random.default_rng(9).standard_normal((60, 10, 1)).astype(np.float32)
    want = V.predict_sequence(cfg, shape, w, st, x, V.REF_WINDOW)
    model = _build(cfg, shape, w, st)
    got = vad.predict_sequence(model, x, vad.preprocess_window([-19, -10, -1, 0, 1, 10, 19]), batch_size=8)      # 22 windows: 8 + 8 + 6
    assert tuple(got.shape) == (60, 1)
    check("predict_sequence", got.cpu().numpy(), want)
    with pytest.raises(ValueError):
        vad.predict_sequence(model, x, V.REF_WINDOW, batch_size=9)
