"""The trainv2 recipe without a GPU: the fp64 oracle (tests/trainv2_oracle.py) pinned against values worked by hand from the reference's
formulas, the class-weight table, the regulariser's flag rule, and the refusals of the new C entry points (which return before any
device call)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import trainv2_oracle as V

# a 2-row, 3-class case: predictions, labels, weights
P = [[0.9, 0.2, 0.6], [0.3, 0.7, 0.05]]
Y = [[1.0, 0.0, 1.0], [0.0, 1.0, 0.0]]
W = [2.0, 0.5, 1.25]


def test_oracle_weighted_bce_by_hand():
    e = 1e-7      # at these predictions float32(1e-7) and 1e-7 give the same value to 1e-13
    want = sum(-(y * math.log(p + e) + (1 - y) * math.log(1 - p + e)) * w for pr, yr in zip(P, Y) for p, y, w in zip(pr, yr, W)) / 6
    _, sl, _ = V.losses_v2(V.t64(P), torch.zeros(2, 9, dtype=torch.float64), V.t64(Y), torch.zeros(2, 9, dtype=torch.float64) + 0.6, V.t64(W))
    assert abs(float(sl) - want) < 1e-12
    assert abs(want - 0.3194380) < 1e-6      # on paper: (0.210721 + 0.111572 + 0.638532 + 0.713350 + 0.178337 + 0.064117) / 6 = 1.916629 / 6


def test_oracle_focal_by_hand():
    a, g = 0.25, 2.0
    f = sum(-y * a * (1 - p) ** g * math.log(p) - (1 - y) * a * p ** g * math.log(1 - p) for pr, yr in zip(P, Y) for p, y in zip(pr, yr)) / 6
    want = f * sum(W) / 3                     # the scalar times the weight row, then the mean (trainv2.py:41)
    _, sl, _ = V.losses_v2(V.t64(P), torch.zeros(2, 9, dtype=torch.float64), V.t64(Y), torch.zeros(2, 9, dtype=torch.float64) + 0.6, V.t64(W),
                           sed_loss="focal")
    assert abs(float(sl) - want) < 1e-12
    # first element alone: -1 * 0.25 * 0.1^2 * ln 0.9 = 2.634e-4
    assert abs(-0.25 * 0.01 * math.log(0.9) - 2.6340e-4) < 1e-8


def test_oracle_label_smoothing_by_hand():
    ls, e = 0.1, 1e-7
    want = 0.0
    for pr, yr in zip(P, Y):
        for p, y, w in zip(pr, yr, W):
            t = y * 0.9 + 0.05                # 1 -> 0.95, 0 -> 0.05
            want += -(t * math.log(p + e) + (1 - t) * math.log(1 - p + e)) * w
    want /= 6
    _, sl, _ = V.losses_v2(V.t64(P), torch.zeros(2, 9, dtype=torch.float64), V.t64(Y), torch.zeros(2, 9, dtype=torch.float64) + 0.6, V.t64(W), ls=ls)
    assert abs(float(sl) - want) < 1e-12
    assert V.smooth(V.t64([1.0, 0.0]), 0.1).tolist() == pytest.approx([0.95, 0.05])
    assert V.smooth(V.t64([1.0, 0.0]), 0.0).tolist() == [1.0, 0.0]


def test_oracle_weighted_mmse_by_hand():
    # row 0: classes 0 and 2 active (unit vectors), row 1: class 1 active; layout [x0 x1 x2 | y0 y1 y2 | z0 z1 z2]
    yd = np.array([[1.0, 0, 0.6, 0, 0, 0.8, 0, 0, 0], [0, 0, 0, 0, 1.0, 0, 0, 0, 0]])
    pd = np.array([[0.5, 0.1, 0.6, 0.1, -0.2, 0.4, 0.0, 0.3, 0.2], [0.2, 0.1, 0.0, 0.0, 0.5, 0.9, -0.4, 0.1, 0.0]])
    # masks m = round(|y|^2) * w: row 0 -> [2, 0, 1.25], row 1 -> [0, 0.5, 0]
    num = 2.0 * (0.5 ** 2 + 0.1 ** 2 + 0.0) + 1.25 * (0.0 + 0.4 ** 2 + 0.2 ** 2) + 0.5 * (0.1 ** 2 + 0.5 ** 2 + 0.1 ** 2)
    den = 3 * (2.0 + 1.25 + 0.5)
    assert abs(num - 0.905) < 1e-12 and den == 11.25
    got = V.mmse_with_cls_weights(V.t64(yd), V.t64(pd), V.t64(W))
    assert abs(float(got) - num / den) < 1e-12
    # without weights it is losses.MMSE
    from oracle import seldnet_oracle as O
    assert float(V.mmse_with_cls_weights(V.t64(yd), V.t64(pd))) == float(O.mmse(V.t64(yd), V.t64(pd)))


def test_oracle_adabelief_three_steps_by_hand():
    """utils.py:162-182 in numpy, step by step, on a 4-element vector."""
    th = np.array([0.5, -0.25, 1.0, 0.0])
    gs = [np.array([0.1, -0.2, 0.0, 0.3]), np.array([0.05, 0.1, -0.4, 0.3]), np.array([-0.2, 0.1, 0.1, 0.0])]
    b1, b2, eps, lr = 0.9, 0.999, 1e-7, 1e-2
    m, v = np.zeros(4), np.zeros(4)
    t_o, m_o, v_o = V.t64(th), V.t64(m), V.t64(v)
    for k, g in enumerate(gs, 1):
        m = m * b1 + g * (1 - b1)                      # :164-166
        dev_ = g - m                                   # :171, the updated m
        v = v * b2 + dev_ * dev_ * (1 - b2)            # :172-174
        lr_t = lr * math.sqrt(1 - b2 ** k) / (1 - b1 ** k)   # :132-138
        th = th - lr_t * m / (np.sqrt(v) + eps)        # :178-180
        t_o, m_o, v_o = V.adabelief(t_o, V.t64(g), m_o, v_o, k, lr, b1, b2, eps)
        np.testing.assert_allclose(t_o.numpy(), th, rtol=0, atol=1e-15)
        np.testing.assert_allclose(m_o.numpy(), m, rtol=0, atol=1e-15)
        np.testing.assert_allclose(v_o.numpy(), v, rtol=0, atol=1e-18)
    # the first step on paper: m = 0.1 g, v = 0.001 (0.9 g)^2, lr_t = lr sqrt(0.001) / 0.1 -> step = lr / 0.9 sign(g) (up to eps), 0 where g = 0
    t1, _, _ = V.adabelief(V.t64([0.5, -0.25, 1.0, 0.0]), V.t64(gs[0]), V.t64(np.zeros(4)), V.t64(np.zeros(4)), 1, lr, b1, b2, eps)
    np.testing.assert_allclose(t1.numpy() - [0.5, -0.25, 1.0, 0.0], [-lr / 0.9, lr / 0.9, 0.0, -lr / 0.9], atol=1e-6)


def test_oracle_agc_decision_by_hand():
    """One clipped and one unclipped unit of a [2, 2] matrix (units = columns, utils.py:75-77)."""
    p = V.t64([[3.0, 0.0], [4.0, 1e-5]])             # column norms 5 and 1e-5 -> max_norm 0.05 and max(1e-5, 1e-3) * 0.01 = 1e-5
    g = V.t64([[0.03, 6e-6], [0.04, 8e-6]])          # column norms 0.05 (not < 0.05: clipped, by a factor of exactly 1) and 1e-5 ...
    g = g * V.t64([[2.0, 0.5]])                      # ... -> 0.1 (clipped to 0.05) and 5e-6 (kept)
    out, ratio = V.agc(p, g)
    np.testing.assert_allclose(ratio.numpy(), [2.0, 0.5], rtol=1e-12)
    np.testing.assert_allclose(out.numpy(), [[0.03, 3e-6], [0.04, 4e-6]], rtol=1e-12)
    # a vector is one unit (utils.py:72-74)
    out, ratio = V.agc(V.t64([3.0, 4.0]), V.t64([0.3, 0.4]))
    np.testing.assert_allclose(out.numpy(), [0.03, 0.04], rtol=1e-12)
    # and the regulariser enters before the norm: g + 2 l2 w
    r = V.reg_agc_adabelief([3.0, 4.0], [0.0, 0.0], [0.0, 0.0], [0.0, 0.0], [(2,)], [1], 1, l2=0.5, clip_factor=0.01)
    np.testing.assert_allclose(r["ratio"], [100.0], rtol=1e-12)          # |2 * 0.5 * w| = 5 against 0.05
    np.testing.assert_allclose(r["g"], [0.03, 0.04], rtol=1e-12)
    r = V.reg_agc_adabelief([3.0, 4.0], [0.0, 0.0], [0.0, 0.0], [0.0, 0.0], [(2,)], [0], 1, l2=0.5, clip_factor=0.0)
    np.testing.assert_array_equal(r["g"], [0.0, 0.0])


def test_oracle_swa_three_updates_by_hand():
    ws = [np.array([1.0, 2.0], np.float32), np.array([2.0, 0.0], np.float32), np.array([6.0, 1.0], np.float32)]
    swa = ws[0].copy()                                # swa.py:26-27, cnt 0 -> 1
    swa = V.swa_update(swa, ws[1], 1)                 # (swa + w) / 2
    np.testing.assert_array_equal(swa, np.array([1.5, 1.0], np.float32))
    swa = V.swa_update(swa, ws[2], 2)                 # (2 swa + w) / 3
    np.testing.assert_array_equal(swa, (np.array([9.0, 3.0], np.float32) / np.float32(3)))
    assert swa.dtype == np.float32
    assert [e for e in range(12) if V.swa_fires(e, 5, 2)] == [4, 6, 8, 10]      # start_epoch 5 is stored as 4 (swa.py:8)
    assert [e for e in range(8) if V.swa_fires(e, 1, 3)] == [0, 3, 6]


def test_default_class_weights():
    from seld_amd import trainv2
    t = np.array([58193, 32794, 29801, 21478, 14822, 9174, 66527, 6740, 9342, 6498, 22218, 49758], np.float64)      # trainv2.py:25-29
    assert trainv2.TRAIN_SAMPLES == tuple(int(v) for v in t) == V.TRAIN_SAMPLES
    w = trainv2.default_cls_weights()
    assert w.dtype == np.float32 and w.shape == (12,)
    np.testing.assert_allclose(w, t.mean() / t, rtol=2e-7)
    assert abs(t.mean() - 27278.75) < 1e-9


def _names(cfg):
    from oracle import seldnet_oracle as O
    return [n for n, _ in O.variable_specs(O.Spec.from_config(cfg))[0]]


def test_regulariser_flag_rule(seldnet_config, xception_config, resnet50_config):
    from seld_amd import trainv2
    heads = ["sed.dense0.kernel", "sed.out.kernel", "doa.dense0.kernel", "doa.out.kernel"]
    flagged = {k: [n for n in _names(cfg) if trainv2.is_regularized(n)] for k, cfg in
               (("seldnet", seldnet_config), ("xception", xception_config), ("resnet50", resnet50_config))}
    assert flagged["seldnet"] == ["conv0.kernel", "conv1.kernel", "conv2.kernel"] + heads      # the list DESIGN.md documents
    assert flagged["xception"] == ["conv0.kernel"] + heads
    rn = [n for n in _names(resnet50_config) if n.startswith("rn") and n.endswith(".kernel")]
    assert len(rn) == 3 * 16 + 4 and flagged["resnet50"] == ["conv0.kernel"] + rn + heads
    for cfg in (seldnet_config, xception_config, resnet50_config):
        for n in _names(cfg):
            assert trainv2.is_regularized(n) == V.is_regularized(n)
            if n.startswith("gru") or n.endswith(("bias", "gamma", "beta", "depthwise_kernel", "pointwise_kernel")):
                assert not trainv2.is_regularized(n), n
    assert sum(n.endswith("depthwise_kernel") for n in _names(xception_config)) == 24


def test_generate_trainstep_refusals():
    from seld_amd import losses, trainv2

    class Fake:
        n_classes = 14

    step = trainv2.generate_trainstep(losses.BinaryCrossentropy(), losses.MMSE_with_cls_weights, (1, 1000))
    with pytest.raises(ValueError, match="class-weight table"):
        step(Fake(), None, None, trainv2.AdaBelief())
    Fake.n_classes = 12
    with pytest.raises(ValueError, match="composed"):      # anything that is not a fused context, modules.ComposedSeldNet included
        step(Fake(), None, None, trainv2.AdaBelief())
    Fake.n_classes = 14
    step = trainv2.generate_trainstep(losses.focal_loss, losses.MMSE_with_cls_weights, (1, 1000), 0.1, cls_weights=np.ones(14))
    with pytest.raises(ValueError, match="composed"):      # explicit weights of the right length pass the table check
        step(Fake(), None, None, trainv2.AdaBelief())
    with pytest.raises(ValueError):
        trainv2.generate_trainstep(losses.MSE, losses.MMSE_with_cls_weights, (1, 1000))
    with pytest.raises(ValueError):
        trainv2.generate_trainstep(losses.BinaryCrossentropy(), losses.MMSE, (1, 1000))
    with pytest.raises(ValueError):
        trainv2.generate_trainstep(losses.BinaryCrossentropy(), losses.MMSE_with_cls_weights, (1, 1000), label_smoothing=1.0)
    o = trainv2.AdaBelief()
    assert (o.learning_rate, o.beta_1, o.beta_2, o.epsilon) == (1e-3, 0.9, 0.999, 1e-7)
    assert (losses.focal_loss.alpha, losses.focal_loss.gamma) == (0.25, 2.0) and losses.focal_loss(gamma=3).gamma == 3.0


def test_v2_entry_points_refuse_bad_arguments(seld_lib):
    """Every refusal below is made before the first device call."""
    from seld_amd import _lib
    INVALID = -1
    q = C.c_void_p(256)      # a non-NULL pointer that is never dereferenced
    cfg = _lib.V2Cfg(_lib.SELD_SED_BCE, 1.0, 1000.0, 0.0, 0.25, 2.0)
    ok = lambda c, nc=12, **kw: seld_lib.seld_k_losses_v2(kw.get("sed", q), q, q, kw.get("y_doa", q), c, kw.get("sloss", q), q, None, None, 2, 10, nc)
    assert ok(None) == INVALID
    assert ok(C.byref(cfg), sed=None) == INVALID and ok(C.byref(cfg), y_doa=None) == INVALID and ok(C.byref(cfg), sloss=None) == INVALID
    assert ok(C.byref(cfg), nc=33) == INVALID and ok(C.byref(cfg), nc=0) == INVALID
    for bad in (dict(sed_loss=2), dict(sed_loss=-1), dict(label_smoothing=1.0), dict(label_smoothing=-0.1), dict(label_smoothing=float("nan"))):
        c2 = _lib.V2Cfg(_lib.SELD_SED_FOCAL, 1.0, 1000.0, 0.0, 0.25, 2.0)
        for k, v in bad.items():
            setattr(c2, k, v)
        assert ok(C.byref(c2)) == INVALID, bad

    def opt(n=100, off=(0, 40), rows=(4, 6), cols=(10, 10), step=1, theta=q, reg=(1, 0), l2=0.0):
        nv = len(off)
        return seld_lib.seld_k_reg_agc_adabelief(theta, q, q, q, n, nv, (C.c_int64 * max(nv, 1))(*off), (C.c_int32 * max(nv, 1))(*rows),
                                                 (C.c_int32 * max(nv, 1))(*cols), (C.c_int32 * max(nv, 1))(*reg), 1e-3, 0.9, 0.999, 1e-7, l2, 0.01, step)
    assert opt(theta=None) == INVALID and opt(step=0) == INVALID and opt(n=0) == INVALID
    assert opt(n=99) == INVALID                    # the second variable ends past the buffer
    assert opt(off=(0, 39)) == INVALID             # overlap
    assert opt(rows=(4, 0)) == INVALID and opt(cols=(0, 10)) == INVALID
    assert opt(off=(), rows=(), cols=(), reg=()) == INVALID
    assert opt(l2=-1.0) == INVALID
    assert seld_lib.seld_k_reg_agc_adabelief(q, q, q, q, 100, 1, None, None, None, None, 1e-3, 0.9, 0.999, 1e-7, 0.0, 0.01, 1) == INVALID

    assert seld_lib.seld_train_fwd_bwd_v2(None, q, q, q, C.byref(cfg), None, None, None, None) == INVALID
    assert seld_lib.seld_set_regularized(None, (C.c_int32 * 1)(1), 1) == INVALID
    assert seld_lib.seld_v2_opt_step(None, 1e-3, 0.9, 0.999, 1e-7, 1e-3, 0.01) == INVALID
    assert seld_lib.seld_swa_update(None) == INVALID and seld_lib.seld_swa_apply(None) == INVALID and seld_lib.seld_swa_count(None) == INVALID
    assert C.sizeof(_lib.V2Cfg) == 4 * (6 + _lib.V2_MAX_CLASSES)
