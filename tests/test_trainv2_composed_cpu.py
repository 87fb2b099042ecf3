"""The trainv2 recipe on composed models without a GPU: the regulariser's flag rule on the composed variable names, the clip-unit mapping, the
refusals of the new stream operators (made before any device call) and the host's draws for seld_aug_v2."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import conv_temporal_oracle as CT
import trainv2_oracle as V
from conftest import ROOT

INVALID, UNSUPPORTED = -1, -2
CONFORMER = ["ffn0a.kernel", "ffn0b.kernel", "mha.query_kernel", "mha.key_kernel", "mha.value_kernel", "mha.projection_kernel", "pw0.kernel",
             "dw.kernel", "pw1.kernel", "ffn1a.kernel", "ffn1b.kernel"]
ONE_DIRECTION = dict(CT.CHAIN2, BLOCK1_ARGS={"depth": 1, "units": 128, "rnn_type": "GRU", "bidirectional": False})


def _names(shape, cfg):
    from seld_amd import modules
    return [(n, sh) for n, _, sh in modules.ConvTemporalNet(shape, cfg, device="meta").variables]


def _flagged(shape, cfg):
    from seld_amd import trainv2
    return [n for n, _ in _names(shape, cfg) if trainv2.is_regularized_composed(n)]


# ------------------------------------------------------------------------------------------------ 1. the regulariser rule
def test_regulariser_rule_on_ss5():
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "SS5.json")))
    want = ["stem.conv.kernel"]
    want += ["b0.mb0.c1.kernel", "b0.mb0.p1_0.kernel", "b0.mb0.s2_0.kernel"]      # the strided block: conv, projection, strided concatenation
    want += ["b0.mb1.c1.kernel", "b0.mb1.p1_0.kernel"]
    want += ["b1.dense0.kernel"]
    want += [f"b2.cf{d}.{n}" for d in (0, 1) for n in CONFORMER] + [f"sed.cf0.{n}" for n in CONFORMER]
    want += ["sed_out.kernel", "doa_out.kernel"]                                   # nothing of the DOA head's Bidirectional GRUs
    got = _flagged((1, 300, 64, 7), cfg)
    assert got == want
    names = [n for n, _ in _names((1, 300, 64, 7), cfg)]
    assert sum(n.startswith("doa.gru") for n in names) == 12 and not any(n.startswith("doa.gru") for n in got)
    assert not any(n.endswith(("bias", "gamma", "beta", "recurrent_kernel")) for n in got)


def test_regulariser_rule_on_the_second_chain_and_a_one_direction_rnn():
    want = ["stem.conv.kernel", "b0.mb0.c0.kernel", "b0.mb0.p0_0.kernel", "b0.mb0.c2.kernel", "b0.mb0.p2_0.kernel", "b0.mb0.p2_1.kernel",
            # BLOCK1 (a Bidirectional LSTM): none; BLOCK2, a Keras MultiHeadAttention (none of its four kernels) and two Conv1D
            "b2.tf0.ffn0.kernel", "b2.tf0.ffn1.kernel",
            "sed_out.kernel", "doa.dense0.kernel", "doa.dense1.kernel", "doa_out.kernel"]
    assert _flagged(CT.CHAIN2_INPUT, CT.CHAIN2) == want
    names = [n for n, _ in _names(CT.CHAIN2_INPUT, CT.CHAIN2)]
    for leaf in ("query", "key", "value", "attention_output"):
        assert f"b2.tf0.mha.{leaf}.kernel" in names
    assert "b1.rnn0.fwd.kernel" in names and "b1.rnn0.bwd.kernel" in names
    # a bare GRU layer has the attribute: its input kernel is regularised, its recurrent kernel and bias are not
    one = _flagged(CT.CHAIN2_INPUT, ONE_DIRECTION)
    assert [n for n in one if n.startswith("b1.")] == ["b1.rnn0.kernel"]
    assert [n for n, _ in _names(CT.CHAIN2_INPUT, ONE_DIRECTION) if n.startswith("b1.")] == ["b1.rnn0.kernel", "b1.rnn0.recurrent_kernel", "b1.rnn0.bias"]


def test_head_major_position_variables_are_regularised():
    from seld_amd import trainv2
    for leaf in ("pos_kernel", "pos_bias_u", "pos_bias_v", "query_kernel", "key_kernel", "value_kernel", "projection_kernel"):
        assert trainv2.is_regularized_composed(f"b1.at0.mha.{leaf}"), leaf
    for leaf in ("projection_bias", "q_bias", "k_bias", "v_bias"):
        assert not trainv2.is_regularized_composed(f"b1.at0.mha.{leaf}"), leaf


def test_fused_rule_is_unchanged(seldnet_config, xception_config, resnet50_config):
    from oracle import seldnet_oracle as O
    from seld_amd import trainv2
    for cfg in (seldnet_config, xception_config, resnet50_config):
        for n, _ in O.variable_specs(O.Spec.from_config(cfg))[0]:
            assert trainv2.is_regularized(n) == V.is_regularized(n) == (n.endswith(".kernel") and not n.startswith("gru")), n


# ------------------------------------------------------------------------------------------------ 2. the unit mapping
def test_unit_mapping():
    from seld_amd import modules
    u = modules.v2_unit_shape
    assert u((384,)) == (384, 1) and u(()) == (1, 1)                 # rank <= 1: one unit
    assert u((2, 384)) == (2, 384)                                    # the GRU's bias: 384 units of two values
    assert u((192, 384)) == (192, 384)
    assert u((4, 192, 24)) == (4, 192 * 24)                           # head-major (H, D, dk): H rows, as the reference is written
    assert u((24, 1, 192)) == (24, 192)                               # the depthwise kernel (k, 1, C)
    assert u((1, 192, 384)) == (1, 192 * 384)
    assert u((7, 7, 7, 32)) == (7 * 7 * 7, 32)
    with pytest.raises(ValueError):
        u((2, 3, 4, 5, 6))
    # every shape of the two test models maps to its own size, and the oracle's norm has `cols` entries
    import torch
    for shape, cfg in ((CT.SS5_SMALL_INPUT, CT.SS5_SMALL), (CT.CHAIN2_INPUT, CT.CHAIN2)):
        for n, sh in _names(shape, cfg):
            r, c = u(sh)
            assert r * c == int(np.prod(sh)) and V.unitwise_norm(torch.zeros(sh)).numel() == c, n


# ------------------------------------------------------------------------------------------------ 3. refusals, with no device
def test_stream_operators_refuse_bad_arguments(seld_lib):
    from seld_amd import _lib
    q = C.c_void_p(256)      # a non-NULL, 8-byte aligned pointer that is never dereferenced
    cfg = _lib.V2Cfg(_lib.SELD_SED_BCE, 1.0, 1000.0, 0.0, 0.25, 2.0)

    def loss(c=None, nc=12, B=2, S=10, **kw):
        a = {k: q for k in ("sed", "doa", "y_sed", "y_doa", "sloss", "dloss", "scratch")}
        a.update(kw)
        return seld_lib.seld_v2_losses(a["sed"], a["doa"], a["y_sed"], a["y_doa"], C.byref(cfg) if c is None else c, a["sloss"], a["dloss"], None,
                                         None, a["scratch"], B, S, nc, None)
    for k in ("sed", "doa", "y_sed", "y_doa", "sloss", "dloss", "scratch"):
        assert loss(**{k: None}) == INVALID, k
    assert seld_lib.seld_v2_losses(q, q, q, q, None, q, q, None, None, q, 2, 10, 12, None) == INVALID
    assert loss(nc=33) == INVALID and loss(nc=0) == INVALID and loss(B=0) == INVALID and loss(S=0) == INVALID
    assert loss(scratch=C.c_void_p(260)) == INVALID                  # the partials are doubles
    for bad in (dict(sed_loss=2), dict(sed_loss=-1), dict(label_smoothing=1.0), dict(label_smoothing=-0.1), dict(label_smoothing=float("nan"))):
        c2 = _lib.V2Cfg(_lib.SELD_SED_FOCAL, 1.0, 1000.0, 0.0, 0.25, 2.0)
        for k, v in bad.items():
            setattr(c2, k, v)
        assert loss(C.byref(c2)) == INVALID, bad
    for r in (1, 64, 65):
        assert seld_lib.seld_v2_losses_scratch(r) == seld_lib.seld_m_losses_scratch(r) == 2 * r + 64 + 4
    assert seld_lib.seld_v2_losses_scratch(0) == -1 and seld_lib.seld_v2_losses_scratch(-3) == -1

    def plan(n=100, off=(0, 40), rows=(4, 6), cols=(10, 10), reg=(1, 0), out=True, null=None):
        nv = len(off)
        arr = [(C.c_int64 * max(nv, 1))(*off), (C.c_int32 * max(nv, 1))(*rows), (C.c_int32 * max(nv, 1))(*cols), (C.c_int32 * max(nv, 1))(*reg)]
        if null is not None:
            arr[null] = None
        p = C.c_void_p(77)
        rc = seld_lib.seld_v2_plan_create(n, nv, *arr, C.byref(p) if out else None)
        assert not out or rc == 0 or p.value is None      # a refused call leaves NULL behind
        return rc
    assert plan(out=False) == INVALID and plan(n=0) == INVALID
    for k in range(4):
        assert plan(null=k) == INVALID
    assert plan(n=99) == INVALID                    # the second variable ends past the buffer
    assert plan(off=(0, 39)) == INVALID             # overlap
    assert plan(rows=(4, 0)) == INVALID and plan(cols=(0, 10)) == INVALID      # an empty variable
    assert plan(off=(), rows=(), cols=(), reg=()) == INVALID                    # an empty table
    seld_lib.seld_v2_plan_destroy(None)            # nothing to free

    def opt(plan_=q, theta=q, g=q, m=q, v=q, step=1, l2=0.0):
        return seld_lib.seld_v2_opt(plan_, theta, g, m, v, 1e-3, 0.9, 0.999, 1e-7, l2, 0.01, step, None)
    for k in ("plan_", "theta", "g", "m", "v"):
        assert opt(**{k: None}) == INVALID, k
    assert opt(step=0) == INVALID and opt(l2=-1.0) == INVALID and opt(l2=float("nan")) == INVALID

    assert seld_lib.seld_v2_swa(None, q, 10, 0, None) == INVALID and seld_lib.seld_v2_swa(q, None, 10, 1, None) == INVALID
    assert seld_lib.seld_v2_swa(q, q, 0, 1, None) == INVALID and seld_lib.seld_v2_swa(q, q, 10, -1, None) == INVALID


def test_aug_v2_refuses_bad_arguments(seld_lib):
    q = C.c_void_p(256)
    B, T, F, Cc, period = 2, 200, 8, 7, 100
    N = B * T // period

    def tab(n, size, off):
        return (C.c_int32 * (n * N))(*([off] * (n * N))), (C.c_int32 * (n * N))(*([size] * (n * N)))

    def aug(x=q, T_=T, Cc_=Cc, nsc=4, n_t=2, n_f=2, t=(3, 5), f=(2, 1), t_null=False, f_null=False):
        to, ts = tab(max(n_t, 1), *t)
        fo, fs = tab(max(n_f, 1), *f)
        if t_null:
            to = ts = None
        if f_null:
            fo = fs = None
        return seld_lib.seld_aug_v2(x, B, T_, F, Cc_, period, q, nsc, to, ts, n_t, fo, fs, n_f, None)
    assert aug(x=None) == INVALID
    assert aug(T_=250) == INVALID                                     # T % period
    assert aug(n_t=0, t_null=True, n_f=17) == INVALID and aug(n_f=0, f_null=True, n_t=17) == INVALID
    assert aug(nsc=8) == INVALID and aug(nsc=-1) == INVALID           # n_shift_ch > C
    assert aug(t_null=True) == INVALID and aug(f_null=True) == INVALID
    assert aug(t=(6, 95)) == INVALID                                  # frames [95, 101) of a 100-frame segment
    assert aug(f=(3, 6)) == INVALID                                   # bins [6, 9) of 8
    assert aug(t=(-1, 5)) == INVALID and aug(f=(1, -1)) == INVALID
    assert aug(Cc_=4096, nsc=4) == UNSUPPORTED                        # F * C = 32768 floats in a frame
    for bad in (dict(B=0), dict(F=0), dict(period=0)):
        a = dict(B=B, F=F, period=period)
        a.update(bad)
        assert seld_lib.seld_aug_v2(q, a["B"], T, a["F"], Cc, a["period"], None, 0, None, None, 0, None, None, 0, None) == INVALID
    # nothing to do: no shift, no masks — returns before any device call
    assert seld_lib.seld_aug_v2(q, B, T, F, Cc, period, None, 4, None, None, 0, None, None, 0, None) == 0
    assert seld_lib.seld_aug_v2(q, B, T, F, Cc, period, q, 0, None, None, 0, None, None, 0, None) == 0


def test_composed_refusals_by_kind():
    from seld_amd import losses, trainv2

    class Fake:
        n_classes = 12

    with pytest.raises(ValueError, match="composed"):
        trainv2.apply_kernel_regularizer(Fake())
    with pytest.raises(ValueError, match="composed"):
        trainv2.SWA(Fake(), 1)
    ts = trainv2.generate_teststep(losses.BinaryCrossentropy(), losses.MMSE_with_cls_weights)
    with pytest.raises(ValueError, match="composed"):
        ts(Fake(), None, None)
    step = trainv2.generate_trainstep(losses.BinaryCrossentropy(), losses.MMSE_with_cls_weights, (1, 1000))
    Fake.n_classes = 14
    with pytest.raises(ValueError, match="class-weight table"):      # the class-weight check still comes first
        step(Fake(), None, None, trainv2.AdaBelief())


# ------------------------------------------------------------------------------------------------ 4. the draws
DRAW_SEED = 2021


def test_v2_draws():
    """10 000 draws of every table entry: sizes in [0, max - 1], offsets in [0, total - size - 1] (tf.random.uniform's maxval is exclusive);
    the shifts are float32 ~ N(0, 0.2^2).  The sample mean of 10 000 such values has a standard deviation of 0.002 and the sample standard
    deviation one of 0.0014: the bounds below are five and seven of those."""
    from seld_amd import transforms
    rng = np.random.default_rng(DRAW_SEED)
    B, nseg, F = 100, 100, 64
    shift, (ts, to), (fs, fo) = transforms.draw_v2(rng, B, nseg, F)
    assert ts.shape == to.shape == (10, B * nseg) and fs.shape == fo.shape == (6, B * nseg) and shift.shape == (B,)
    for a in (ts, to, fs, fo):
        assert a.dtype == np.int32
    assert ts.min() == 0 and ts.max() == 5 and fs.min() == 0 and fs.max() == 7
    assert to.min() == 0 and (to <= 100 - ts - 1).all() and (to == 100 - ts - 1).any()
    assert fo.min() == 0 and (fo <= 64 - fs - 1).all() and (fo == 64 - fs - 1).any()
    sh = np.concatenate([transforms.draw_v2(rng, 100, 1, F, time=(6, 0), freq=(8, 0))[0] for _ in range(100)])
    assert sh.dtype == np.float32 and sh.size == 10000
    assert abs(float(sh.mean())) < 0.01 and 0.19 <= float(sh.std()) <= 0.21
    # other sizes reach the tables' shapes
    s2, (a, b), (c, d) = transforms.draw_v2(rng, 3, 2, 8, time=(4, 2), freq=(3, 0), period=50)
    assert a.shape == b.shape == (2, 6) and c.shape == d.shape == (0, 6) and (a + b <= 49).all()


# ------------------------------------------------------------------------------------------------ 5. the GPU tests' inputs
def test_optimizer_case_decisions_are_safe():
    """the table of tests/test_trainv2_composed_gpu.py::test_m_v2_opt: offsets as documented, and two oracle steps per (l2, clip) whose units
    lie on both sides of the clip decision, none within 1e-3 of it — the seed was chosen so"""
    import trainv2_composed_cases as K
    off = np.cumsum([0] + [int(np.prod(s)) for s in K.OPT_SHAPES])
    assert list(off[:-1]) == K.OPT_OFFSETS and off[-1] == K.OPT_N
    assert [K.rows_cols(s) for s in K.OPT_SHAPES] == [(36, 8), (13, 1), (2, 384), (4, 144), (5, 10), (7, 1), (130, 30), (3, 1)]
    assert any(o < 4096 < o + int(np.prod(s)) for o, s in zip(K.OPT_OFFSETS, K.OPT_SHAPES))
    assert {o % 4 for o in K.OPT_OFFSETS} == {0, 1, 2, 3}
    from seld_amd import modules
    assert [modules.v2_unit_shape(s) for s in K.OPT_SHAPES] == [K.rows_cols(s) for s in K.OPT_SHAPES]
    for l2 in (0.0, 1e-3):
        th = K.opt_weights().astype(np.float64)
        m, v = np.zeros_like(th), np.zeros_like(th)
        for step in (1, 2):
            r = V.reg_agc_adabelief(th, K.opt_grads(th, step), m, v, K.OPT_SHAPES, K.OPT_REG, step, l2=l2)
            assert K.ratios_are_safe(r["ratio"]) and r["ratio"].size == 8 + 1 + 384 + 144 + 10 + 1 + 30 + 1
            th, m, v = r["theta"].astype(np.float32), r["m"].astype(np.float32), r["v"].astype(np.float32)


def test_aug_v2_numpy_restatement_by_hand():
    import trainv2_composed_cases as K
    x = np.ones((1, 4, 3, 2), np.float32)
    out = K.aug_v2_numpy(x, [0.5], 1, (np.array([[2]]), np.array([[1]])), (np.array([[1]]), np.array([[2]])), 4)
    want = np.ones((1, 4, 3, 2), np.float32)
    want[..., 0] = 1.5
    want[0, 1:3] = 0      # frames 1, 2
    want[0, :, 2] = 0     # bin 2
    assert np.array_equal(out, want) and np.array_equal(x, np.ones((1, 4, 3, 2), np.float32))
    for shape, period in (((2, 200, 8, 7), 100), ((1, 100, 5, 10), 100)):
        B, T, F, _ = shape
        shift, (ts, to), (fs, fo) = K.aug_draws(B, T // period, F, period, 10, 6, seed=3)
        assert (ts[:, 0] == 0).any() and (to[:, 0] == 0).any() and (to[:, 0] + ts[:, 0] == period).any() and (fo[:, 0] + fs[:, 0] == F).any()
        assert (fs == F).any() == (B * T // period > 1)
