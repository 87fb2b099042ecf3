"""models.vad_architecture on the device: the head's kernels (seld_amd/csrc/vadarch.hip) through the C ABI, then modules.VadArchNet and the two
recipes against the fp64 restatement tests/vadarch_oracle.py at the project's bar (helpers.check: max|d| / max|ref| <= 1e-4).
tests/test_vadarch_cpu.py asserts, on the same cases, that the model cases keep their relu margins and that plain fp32 stays within half the bar.

Every operand of a kernel call sits in a NaN-filled allocation (test_attention_gpu._Window, as tests/test_step_tail_gpu.py uses it): outputs
start as NaN, inputs must keep their bits, and no float outside a window may change.  Gradients that are zero by mathematics (a convolution
bias in front of training-mode BatchNormalization) are asserted absolutely: |g| <= 1e-4 max|gradient|."""
import ctypes as C
import functools
import json

import numpy as np
import pytest
import torch

import vadarch_oracle as VO
from helpers import check, rel_err
from test_attention_gpu import _Window
from test_vadarch_cpu import refusal_checks

pytestmark = pytest.mark.gpu

FRONT, BACK = 68, 36      # floats around every window; multiples of 4: the float4 forms need 16-byte aligned operands


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _in(a, front=FRONT):
    a = np.ascontiguousarray(a, np.float32)
    a = a.reshape(a.shape[0], -1) if a.ndim > 1 else a.reshape(1, -1)
    w = _Window(a.shape[0], a.shape[1], front=front, back=BACK, data=a)
    w.snapshot()
    return w


def _out(rows, cols, front=FRONT):
    return _Window(rows, cols, front=front, back=BACK)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class _Head:
    """one forward and one backward call of the head on (x, w, b, y) -> numpy p, loss, dx (None without), dw, db"""

    def __init__(self, lib, x, w, b, y, weight=1.0, want_dx=True, front=FRONT, scratch_floats=None):
        rows, D = x.shape
        U = w.shape[1]
        wx, ww, wb, wy = _in(x, front), _in(w), _in(b), _in(y)
        wp = _out(rows, U)
        assert lib.seld_vadarch_head_fwd(wx.ptr(), ww.ptr(), wb.ptr(), wp.ptr(), rows, D, U, _stream()) == 0
        torch.cuda.synchronize()
        wp.assert_band("p")
        self.p = wp.numpy()
        wp.snapshot()
        n = int(lib.seld_vadarch_head_bwd_scratch(rows, D, U))
        assert n >= D * U + 1 + U and (scratch_floats is None or n <= scratch_floats)
        scratch = _out(1, n if scratch_floats is None else scratch_floats)      # scratch_floats: the buffer of a larger batch
        wl, wdw, wdb = _out(1, 1), _out(D, U), _out(1, U)
        wdx = _out(rows, D, front) if want_dx else None
        rc = lib.seld_vadarch_head_bwd(wx.ptr(), ww.ptr(), wp.ptr(), wy.ptr(), wl.ptr(), wdx.ptr() if want_dx else None, wdw.ptr(), wdb.ptr(),
                                       scratch.ptr(), rows, D, U, weight, _stream())
        assert rc == 0
        torch.cuda.synchronize()
        for name, win in (("x", wx), ("w", ww), ("b", wb), ("y", wy), ("p", wp)):
            win.assert_unchanged(name)
        for name, win in (("loss", wl), ("dw", wdw), ("db", wdb), ("scratch", scratch)) + ((("dx", wdx),) if want_dx else ()):
            win.assert_band(name)
        self.loss, self.dw, self.db = float(wl.numpy()[0, 0]), wdw.numpy(), wdb.numpy()[0]
        self.dx = wdx.numpy() if want_dx else None


@functools.lru_cache(maxsize=None)
def _head_reference(rows, D, U):
    x, w, b, y = VO.head_inputs(rows, D, U)
    return x, w, b, y, VO.head_reference(x, w, b, y, 0.75)


@pytest.mark.parametrize("rows,D,U", VO.HEAD_CASES)
def test_head_against_fp64(seld_lib, rows, D, U):
    x, w, b, y, ref = _head_reference(rows, D, U)
    got = _Head(seld_lib, x, w, b, y, 0.75)
    check("p", got.p, ref["p"])
    check("loss", [got.loss], [ref["loss"]])
    check("dx", got.dx, ref["dx"])
    check("dw", got.dw, ref["dw"])
    check("db", got.db, ref["db"])
    # dx = NULL: the head on the data — the other outputs keep their bits
    nodx = _Head(seld_lib, x, w, b, y, 0.75, want_dx=False)
    assert nodx.dx is None and np.array_equal(_bits(nodx.dw), _bits(got.dw)) and np.array_equal(_bits(nodx.db), _bits(got.db))
    assert np.array_equal(_bits([nodx.loss]), _bits([got.loss]))
    # a second run gives the same bits
    again = _Head(seld_lib, x, w, b, y, 0.75)
    for name in ("p", "dx", "dw", "db"):
        assert np.array_equal(_bits(getattr(again, name)), _bits(getattr(got, name))), name
    assert np.array_equal(_bits([again.loss]), _bits([got.loss]))


def test_head_past_the_chunk_cap_on_the_scratch_of_the_largest_batch(seld_lib):
    """rows > 32768: the chunk count stays at its cap, chunks without rows add zeros, and a smaller batch fits the scratch the largest one
    was sized for (the band behind the scratch window keeps its NaNs)"""
    (R, D, U), (r, _, _) = VO.CAPPED_CASES
    n = int(seld_lib.seld_vadarch_head_bwd_scratch(R, D, U))
    assert n == 1024 * (D * U + 1 + U) == int(seld_lib.seld_vadarch_head_bwd_scratch(r, D, U))
    for rows in (R, r):
        x, w, b, y, ref = _head_reference(rows, D, U)
        got = _Head(seld_lib, x, w, b, y, 0.75, scratch_floats=n)
        for name in ("p", "dx", "dw", "db"):
            check(f"{name} at {rows} rows", getattr(got, name), ref[name])
        check(f"loss at {rows} rows", [got.loss], [ref["loss"]])


@pytest.mark.parametrize("D,U", [(64, 8), (63, 1), (257, 1), (80, 1)])
def test_head_forward_order_is_the_shapes_alone(seld_lib, D, U):
    """the same rows at rows = 64 and rows = 65 (another grid), and behind an operand that is not 16-byte aligned (the scalar loads)"""
    x, w, b, y = VO.head_inputs(65, D, U)
    full = _Head(seld_lib, x, w, b, y)
    part = _Head(seld_lib, x[:64], w, b, y[:64])
    assert np.array_equal(_bits(full.p[:64]), _bits(part.p))
    odd = _Head(seld_lib, x, w, b, y, front=FRONT + 1)
    assert np.array_equal(_bits(odd.p), _bits(full.p))
    assert np.array_equal(_bits(odd.dx), _bits(full.dx)) and np.array_equal(_bits(odd.dw), _bits(full.dw))


def test_head_saturated_logits(seld_lib):
    x, w, b, y = VO.saturated_inputs()
    got = _Head(seld_lib, x, w, b, y)
    assert got.p[0, 0] == 1.0 and got.p[1, 0] == 1.0 and 0.0 <= got.p[0, 1] < 1e-7 and 0.0 <= got.p[1, 1] < 1e-7
    loss, dz, dx, dw, db = VO.head_backward(x, w, got.p.astype(np.float64), y)
    assert np.isfinite(got.loss) and (dz[:2] == 0).all()
    assert (got.dx[:2] == 0).all()      # dz == 0 exactly where the clip is active: those rows' dx is dz w^T
    check("loss", [got.loss], [loss])
    check("dx", got.dx, dx)
    check("dw", got.dw, dw)
    check("db", got.db, db)
    # seld_vad_bce decides the same elements
    p, yy = torch.as_tensor(got.p).cuda(), torch.as_tensor(y.astype(np.float32)).cuda()
    dp, l2 = torch.empty_like(p), torch.empty((), device="cuda")
    scratch = torch.empty(int(seld_lib.seld_vad_bce_scratch(p.numel())), device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())
    assert seld_lib.seld_vad_bce(ptr(p), ptr(yy), ptr(l2), ptr(dp), ptr(scratch), p.numel(), 1.0, 0, _stream()) == 0
    torch.cuda.synchronize()
    assert (dp[:2] == 0).all() and (dp[2:] != 0).all()
    check("loss against seld_vad_bce", [got.loss], [float(l2)])


def test_head_refusals_beside_a_live_device(seld_lib):
    x, w, b, y, ref = _head_reference(7, 3, 1)
    good = torch.zeros(64, device="cuda")
    torch.cuda.synchronize()
    refusal_checks(seld_lib, C.c_void_p(good.data_ptr()))
    torch.cuda.synchronize()
    assert float(good.abs().sum()) == 0.0      # nothing was launched on it
    check("p after the refusals", _Head(seld_lib, x, w, b, y, 0.75).p, ref["p"])


# ---------------------------------------------------------------- the model
def _build(cfg, shape, w, st, **kw):
    from seld_amd import models
    m = models.vad_architecture(shape, cfg, **kw)
    m.set_weights(w, st)
    return m


@functools.lru_cache(maxsize=None)
def _model_reference(name):
    cfg, shape, w, st, x, y, _ = VO.model_case(name)
    return VO.train_step(cfg, shape, w, st, x, y)


def _check_grads(name, cfg, shape, got, ref):
    tr, _ = VO.variable_specs(cfg, shape)
    zero, off, top = VO.zero_bias_names(cfg, shape), 0, np.abs(ref).max()
    for n, sh in tr:
        k = int(np.prod(sh))
        if n in zero:
            assert np.abs(got[off:off + k]).max() <= 1e-4 * top, n
        else:
            check(f"{name} d {n}", got[off:off + k], ref[off:off + k])
        off += k


class _Step:
    """a train step whose optimizer does nothing: forward, loss, backward"""
    learning_rate, beta_1, beta_2, epsilon = 0.0, 0.9, 0.999, 1e-7


@functools.lru_cache(maxsize=None)
def _model_run(name, fused):
    cfg, shape, w, st, x, y, _ = VO.model_case(name)
    m = _build(cfg, shape, w, st, fused_head=fused)
    assert m.fused == fused
    pred, loss = m.train_step(x, y, _Step())
    torch.cuda.synchronize()
    return pred.cpu().numpy(), float(loss), m.get_grads(), m.get_weights()[1], m(x).cpu().numpy()


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name", ["a", "b"])
def test_model_against_fp64(name, fused):
    cfg, shape, w, st, x, y, _ = VO.model_case(name)
    ref = _model_reference(name)
    pred, loss, grads, state, inf = _model_run(name, fused)
    assert pred.shape == ref["pred"].shape == (3, 7)
    check("prediction", pred, ref["pred"])
    check("loss", [loss], [ref["loss"]])
    _check_grads(name, cfg, shape, grads, ref["grad"])
    if len(state):
        check("moving statistics", state, ref["new_state"])
    # inference with the NEW moving statistics (the step's learning rate is 0: the weights are the old ones)
    check("inference", inf, VO.infer(cfg, shape, w, ref["new_state"], x))


@pytest.mark.parametrize("name", ["a", "b"])
def test_fused_and_composed_heads_agree(name):
    """both are fp32 with different summation orders: 1e-5 on the loss and on every variable's gradient"""
    cfg, shape, *_ = VO.model_case(name)
    _, lf, gf, _, _ = _model_run(name, True)
    _, lc, gc, _, _ = _model_run(name, False)
    tr, _ = VO.variable_specs(cfg, shape)
    zero, off, top = VO.zero_bias_names(cfg, shape), 0, np.abs(gc).max()
    print(f"[heads] {name} loss fused {lf!r} composed {lc!r}")
    assert abs(lf - lc) <= 1e-5 * abs(lc)
    for n, sh in tr:
        k = int(np.prod(sh))
        if n in zero:
            assert np.abs(gf[off:off + k] - gc[off:off + k]).max() <= 1e-5 * top, n
        else:
            e = rel_err(gf[off:off + k], gc[off:off + k])
            print(f"[heads] {name} {n:24s} fused against composed {e:.3e}")
            assert e <= 1e-5, (n, e)
        off += k


def test_label_shape_is_checked():
    cfg, shape, w, st, x, y, _ = VO.model_case("a")
    m = _build(cfg, shape, w, st)
    with pytest.raises(ValueError, match="label shape"):
        m.train_step(x, y[:, :6], _Step())
    with pytest.raises(ValueError, match="label shape"):
        m.test_step(x, y[..., None])
    p, loss = m.test_step(x[:2], y[:2])      # a smaller batch
    assert p.shape == (2, 7)
    check("test_step loss", [float(loss)], [float(VO.bce(torch.tensor(y[:2]), torch.tensor(VO.infer(cfg, shape, w, st, x[:2]))))])


def test_dropout_draws_the_oracle_masks():
    from seld_amd import modules
    cfg, shape, w, st, x, y, _ = VO.model_case("a_drop")
    m = _build(cfg, shape, w, st)
    assert m.body[0].drop.rate == 0.5 and m.body[0].drop.base == modules.DROP_STREAM0
    m.dropout_step = 5
    p5 = m(x, training=True).cpu().numpy()
    p6 = m(x, training=True).cpu().numpy()
    assert m.dropout_step == 7
    for step, got in ((5, p5), (6, p6)):
        check(f"training forward, step {step}", got, VO.train_step(cfg, shape, w, st, x, y, step=step, seed=m.dropout_seed)["pred"])
    assert np.abs(p5 - p6).max() > 1e-3      # two training forwards differ
    # the step: the gradients carry the same masks
    m.dropout_step = 9
    _, loss = m.train_step(x, y, _Step())
    ref = VO.train_step(cfg, shape, w, st, x, y, step=9, seed=m.dropout_seed)
    check("loss under dropout", [float(loss)], [ref["loss"]])
    _check_grads("a_drop", cfg, shape, m.get_grads(), ref["grad"])
    # inference draws nothing: the rate-0 model's bits
    plain = _build(VO.CFG_A, shape, w, st)
    assert torch.equal(m(x).view(torch.int32), plain(x).view(torch.int32)) and m.dropout_step == 10


@pytest.mark.parametrize("name", ["a", "b"])
def test_two_adam_steps(name):
    from seld_amd import train
    cfg, shape, w, st, x, y, _ = VO.model_case(name)
    lr = 1e-3
    rw, rst, rlosses = VO.adam_steps(cfg, shape, w, st, [(x, y), (x, y)], lr=lr)
    m = _build(cfg, shape, w, st)
    losses = [float(m.train_step(x, y, train.Adam(lr))[1]) for _ in range(2)]
    gw, gst = m.get_weights()
    check("adam losses", losses, rlosses)
    assert losses[1] < losses[0]      # the same batch: the first step lowers its loss
    if len(st):
        check("adam moving statistics", gst, rst)
    tr, _ = VO.variable_specs(cfg, shape)
    zero, off = VO.zero_bias_names(cfg, shape), 0
    for n, sh in tr:
        k = int(np.prod(sh))
        if n in zero:      # a gradient of rounding noise, which Adam normalises to a step of up to lr: held to Adam's bound
            assert np.abs(gw[off:off + k] - w[off:off + k]).max() <= 2 * lr * 1.0001, n
        else:
            check(f"adam {n}", gw[off:off + k], rw[off:off + k])
            assert np.abs(gw[off:off + k] - w[off:off + k]).max() > 0.5 * lr, n      # and it moved
        off += k


def test_adabelief_step_runs_on_the_v2_optimizer():
    import trainv2_oracle as T2
    from seld_amd import trainv2
    cfg, shape, w, st, x, y, _ = VO.model_case("a")
    m = _build(cfg, shape, w, st)
    _, l0 = m.train_step(x, y, trainv2.AdaBelief(1e-3))
    torch.cuda.synchronize()
    g = torch.tensor(_model_reference("a")["grad"])
    want, _, _ = T2.adabelief(torch.tensor(w, dtype=torch.float64), g, torch.zeros_like(g), torch.zeros_like(g), 1, lr=1e-3)
    gw = m.get_weights()[0]
    off = 0
    for n, sh in VO.variable_specs(cfg, shape)[0]:
        k = int(np.prod(sh))
        check(f"adabelief {n}", gw[off:off + k], want.numpy()[off:off + k])
        assert np.abs(gw[off:off + k] - w[off:off + k]).max() > 0.5e-3, n
        off += k
    assert float(m.test_step(x, y)[1]) < float(l0)
    m.close()


# ---------------------------------------------------------------- the recipes
def _synthetic_pairs(n=4, seed=0):
    """utterances whose label is a function of the features: frames of speech are louder"""
    rng = np.random.default_rng(seed)
    pairs = []
    for i in range(n):
        frames = 60 + 7 * i
        y = (np.sin(np.arange(frames) / 4.0 + i) > 0).astype(np.float32)
        x = (0.2 * rng.standard_normal((frames, 80, 1)) + y[:, None, None]).astype(np.float32)
        pairs.append((x, y))
    return pairs


NAS_CFG = {"flatten": False, "last_unit": 1, "BLOCK0": "simple_dense_stage", "BLOCK0_ARGS": {"depth": 2, "units": 16, "activation": "relu",
                                                                                            "dropout_rate": 0.2}}


def test_train_vad_baseline_trains_vad_architecture(tmp_path):
    from seld_amd import modules, train_vad_baseline as T, vad
    pairs = _synthetic_pairs()
    window = [-19, -10, -1, 0, 1, 10, 19]
    trainset = T.prepare_dataset(pairs, window, 4, train=True, n_repeat=3, rng=np.random.default_rng(1))
    valset = T.prepare_dataset(pairs, window, 4)
    name = str(tmp_path / "vadarch_ckpt")
    model, hist = T.train_and_eval(NAS_CFG, [4, 7, 80, 1], trainset, valset, epochs=2, name=name, model="vad_architecture")
    assert isinstance(model, modules.VadArchNet)
    assert sorted(hist) == sorted(["loss", "val_auc", "val_precision", "val_recall", "val_f1", "val_binary_accuracy"])
    assert all(len(v) == 2 for v in hist.values()) and np.isfinite(hist["loss"]).all() and all(0.0 <= a <= 1.0 for a in hist["val_auc"])
    z = np.load(name + ".npz")
    w, _ = model.get_weights()      # the best checkpoint was reloaded
    for n_, o, sh in model.variables:
        assert np.array_equal(w[o:o + int(np.prod(sh))].reshape(sh), z[n_]), n_
    got = T.evaluate_pairs(model, pairs, window, 4)
    assert sorted(got) == ["auc", "binary_accuracy", "f1", "precision", "recall"] and all(np.isfinite(v) for v in got.values())
    seq = vad.predict_sequence(model, pairs[0][0], vad.preprocess_window(window), 4)
    assert tuple(seq.shape) == (len(pairs[0][1]),)
    # the default model is unchanged
    m2, h2 = T.train_and_eval({"T": 2, "dropout_rate": 0.0}, [4, 7, 80, 1], trainset, valset, epochs=1, name=str(tmp_path / "sta"))
    assert isinstance(m2, vad.SpectroTemporalVAD) and len(h2["loss"]) == 1


def test_nas_vad_main_writes_and_resumes(tmp_path):
    from seld_amd import nas_vad
    pairs = _synthetic_pairs()
    files = {}
    for split, ps in (("train", pairs), ("test", pairs[:2])):
        files[split] = str(tmp_path / f"{split}.npz")
        np.savez(files[split], **{f"{c}{i}": a for i, p in enumerate(ps) for c, a in zip("xy", p)})
    out = str(tmp_path / "vad_results.json")
    argv = ["--json_fname", out, "--train", files["train"], "--test", files["test"], "--batch_size", "8", "--n_repeat", "2", "--n_blocks", "2",
            "--min_flops", "1000", "--max_flops", "2000000"]
    res = nas_vad.main(argv + ["--n_samples", "2"])
    saved = json.load(open(out))
    assert sorted(k for k in saved if k.isdigit()) == ["000", "001"] and saved["train_config"]["n_samples"] == 2
    for k in ("000", "001"):
        perf = saved[k]["perf"]
        assert {"loss", "val_loss", "val_auc", "val_binary_accuracy", "val_precision", "val_recall", "flops", "params", "time"} <= set(perf)
        assert np.isfinite(perf["loss"][0]) and 1000 <= perf["flops"] <= 2000000
        assert nas_vad.plan(saved[k]["config"], [7, 80, 1]).complexity() == {"flops": perf["flops"], "params": perf["params"]}
    assert sorted(k for k in res if k.isdigit()) == ["000", "001"]
    first = {k: saved[k] for k in ("000", "001")}
    nas_vad.main(argv + ["--n_samples", "3"])      # resumes at index 2
    saved = json.load(open(out))
    assert sorted(k for k in saved if k.isdigit()) == ["000", "001", "002"] and {k: saved[k] for k in ("000", "001")} == first
    with pytest.raises(ValueError, match="different train_config"):
        nas_vad.main(argv[:-2] + ["--max_flops", "3000000", "--n_samples", "3"])
