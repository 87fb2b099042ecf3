"""CPU checks of the recurrent block (reference modules.RNN_block / RNN_stage, modules.py:64-83, 322-347): tests/rnn_oracle.py against torch.nn.LSTM /
torch.nn.GRU and the merges' closed forms, the configuration rules of seld_amd.modules.check_rnn_config, the C ABI of the six new operators, and —
the margin under tests/test_rnn_gpu.py's 1e-4 bar — a plain fp32 evaluation of every GPU case within 5e-5 of fp64 (helpers.rel_err)."""
import copy
import os
import re

import numpy as np
import pytest
import torch

import rnn_oracle as R
from conftest import ROOT
from helpers import rel_err
from oracle import seldnet_oracle as O

NEW_SYMBOLS = ("seld_rnn_lstm_fwd", "seld_rnn_lstm_bwd", "seld_rnn_gru_fwd", "seld_rnn_gru_bwd", "seld_rnn_merge_fwd", "seld_rnn_merge_bwd")
FP32_MARGIN = 5e-5


def _gates(a, order, u=128):
    """re-order the gate blocks of the last axis: `order` lists, for each block of the result, the block of `a` it takes"""
    return torch.cat([a[..., k * u:(k + 1) * u] for k in order], -1)


def test_oracle_lstm_matches_torch_nn_lstm():
    """torch.nn.LSTM: gate order i | f | g | o (Keras': i | f | c | o, the same), weights [4u, in] = kernel^T, TWO biases (Keras' one = their sum)"""
    torch.manual_seed(0)
    B, S, D, u = 3, 9, 20, 128
    net = torch.nn.LSTM(D, u, batch_first=True, bidirectional=True).double()
    x = torch.randn(B, S, D, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(B, S, 2 * u, dtype=torch.float64)
    y, _ = net(x)
    (gx,) = torch.autograd.grad((y * dy).sum(), x)
    hs = []
    for d, sfx in enumerate(("", "_reverse")):
        k, r = getattr(net, "weight_ih_l0" + sfx).T, getattr(net, "weight_hh_l0" + sfx).T
        b = getattr(net, "bias_ih_l0" + sfx) + getattr(net, "bias_hh_l0" + sfx)
        hs.append(R.lstm_direction(x, k, r, b, bool(d)))
    mine = R.merge(hs[0], hs[1], "concat")
    (gm,) = torch.autograd.grad((mine * dy).sum(), x)
    assert rel_err(mine.detach().numpy(), y.detach().numpy()) <= 1e-10
    assert rel_err(gm.numpy(), gx.numpy()) <= 1e-10


def test_oracle_gru_matches_torch_nn_gru():
    """torch.nn.GRU: gate order r | z | n (Keras': z | r | h), h' = (1 - z) n + z h and the reset gate applied AFTER the recurrent product with its
    bias inside (Keras reset_after=True); bias [2, 3u] = (bias_ih, bias_hh) re-ordered"""
    torch.manual_seed(1)
    B, S, D, u = 3, 9, 20, 128
    net = torch.nn.GRU(D, u, batch_first=True, bidirectional=True).double()
    x = torch.randn(B, S, D, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(B, S, 2 * u, dtype=torch.float64)
    y, _ = net(x)
    (gx,) = torch.autograd.grad((y * dy).sum(), x)
    hs, hs2 = [], []
    for d, sfx in enumerate(("", "_reverse")):
        k, r = (_gates(getattr(net, n + sfx).T, (1, 0, 2)) for n in ("weight_ih_l0", "weight_hh_l0"))
        b = torch.stack([_gates(getattr(net, n + sfx), (1, 0, 2)) for n in ("bias_ih_l0", "bias_hh_l0")])
        hs.append(O.gru_direction(x, k, r, b, bool(d)))
        hs2.append(R.gru_recurrence(x @ k + b[0], r, b[1], bool(d)))      # the oracle's own step loop (the one that exposes dgh)
    mine = R.merge(hs[0], hs[1], "concat")
    (gm,) = torch.autograd.grad((mine * dy).sum(), x)
    assert rel_err(mine.detach().numpy(), y.detach().numpy()) <= 1e-10
    assert rel_err(gm.numpy(), gx.numpy()) <= 1e-10
    assert rel_err(R.merge(hs2[0], hs2[1], "concat").detach().numpy(), y.detach().numpy()) <= 1e-10


def test_gru_probe_gradient_is_the_recurrent_side_gradient():
    """dgh (the probe's gradient) gives the recurrent kernel's and recurrent bias's gradients: dU = h_prev^T dgh, dbias[1] = colsum dgh"""
    ins = R.recurrence_inputs("gru", 2, 10)
    for d in (0, 1):
        t = lambda a: torch.tensor(a, dtype=torch.float64)
        U, brec = t(ins["U"][d]).requires_grad_(), t(ins["brec"][d]).requires_grad_()
        h = R.gru_recurrence(t(ins["gx"][d]), U, brec, bool(d))
        gU, gb = torch.autograd.grad((h * t(ins["dh"][d])).sum(), (U, brec))
        ref = R.gru_reference(ins, dirs=(d,))
        hh, dgh = ref["h"][0], ref["dgh"][0]
        hp = np.zeros_like(hh)
        if d == 0:
            hp[:, 1:] = hh[:, :-1]
        else:
            hp[:, :-1] = hh[:, 1:]
        assert rel_err(np.einsum("bsu,bsg->ug", hp, dgh), gU.numpy()) <= 1e-10
        assert rel_err(dgh.sum((0, 1)), gb.numpy()) <= 1e-10


@pytest.mark.parametrize("mode", R.MERGES)
def test_merges_and_their_gradients_match_the_closed_forms(mode):
    hf, hb, dout = (a.astype(np.float64) for a in R.merge_inputs(5, 3, mode))
    y, ga, gb = R.merge_reference(hf, hb, dout, mode)
    want = {"mul": lambda: (hf * hb, dout * hb, dout * hf), "ave": lambda: ((hf + hb) / 2, dout / 2, dout / 2), "sum": lambda: (hf + hb, dout, dout),
            "concat": lambda: (np.concatenate([hf, hb], 1), dout[:, :3], dout[:, 3:])}[mode]()
    for got, ref in zip((y, ga, gb), want):
        assert np.abs(got - ref).max() <= 1e-15


# ---------------------------------------------------------------- configuration rules
def test_check_rnn_config_refusals():
    from seld_amd import modules
    ok = {"units": 128, "depth": 2}
    modules.check_rnn_config(ok, True)
    modules.check_rnn_config({"units": 128})
    for bad, stage, what in (({"depth": 2}, True, "missing 'units'"), ({"units": 128}, True, "missing 'depth'"), ({}, False, "missing 'units'"),
                             ({"units": 64}, False, "the recurrence kernels are built for 128 units"),
                             ({"units": 128, "dropout_rate": 0.3}, False, "dropout"),
                             ({"units": 128, "merge_mode": None}, False, "merge_mode"), ({"units": 128, "merge_mode": "avg"}, False, "merge_mode"),
                             ({"units": 128, "bidirectional": True, "merge_mode": "max"}, False, "merge_mode")):
        with pytest.raises(ValueError, match=what):
            modules.check_rnn_config(bad, stage)
    # bidirectional=False: merge_mode is ignored, whatever it is (modules_test.py:230 passes None)
    modules.check_rnn_config({"units": 128, "bidirectional": False, "merge_mode": None})
    modules.check_rnn_config({"units": 128, "bidirectional": False, "merge_mode": "avg"})


def test_check_rnn_config_accepts_the_references_test_configs_at_128_units():
    """modules_test.py:46-73, 226-242 with units 128.  Two of the three ask for dropout_rate 0.3, which this path refuses by the rule above: they are
    accepted with the rate set to 0, and refused as written for the rate alone."""
    from seld_amd import modules
    for cfg, stage in R.REFERENCE_CONFIGS:
        c = dict(copy.deepcopy(cfg), units=128)
        if c["dropout_rate"]:
            with pytest.raises(ValueError, match="dropout"):
                modules.check_rnn_config(c, stage)
        c["dropout_rate"] = 0.0
        modules.check_rnn_config(c, stage)
        (modules.RNN_stage if stage else modules.RNN_block)(c)      # the factories raise configuration errors without a device
        with pytest.raises(ValueError, match="128 units"):
            (modules.RNN_stage if stage else modules.RNN_block)(dict(c, units=64))


def test_rnn_second_names_factories_and_the_fused_refusal(seldnet_config):
    from seld_amd import models, modules
    assert modules.RNN_SECOND == ("RNN_block", "RNN_stage")
    assert modules.COMPOSED_SECOND == ("bidirectional_GRU_block", "transformer_encoder_block", "transformer_encoder_stage")
    assert callable(modules.RNN_block) and callable(modules.RNN_stage)
    assert "RNN_stage" in models.seldnet.__doc__
    bad = copy.deepcopy(seldnet_config)
    bad["SECOND"], bad["SECOND_ARGS"] = "RNN_stage", {"depth": 2, "units": 128}
    with pytest.raises(ValueError):      # the fused contexts know bidirectional_GRU_block alone
        models._arch_from_config(bad, 7, 64)


def test_out_dim_and_variable_shapes_of_the_oracle():
    assert R.out_dim({"units": 128, "merge_mode": "concat"}) == 256 and R.out_dim({"units": 128, "merge_mode": "concat", "bidirectional": False}) == 128
    tr = R.stage_specs(40, {"units": 128, "rnn_type": "LSTM", "merge_mode": "concat"}, 2)
    assert tr[:3] == [("rnn0.fwd.kernel", (40, 512)), ("rnn0.fwd.recurrent_kernel", (128, 512)), ("rnn0.fwd.bias", (512,))]
    assert tr[6] == ("rnn1.fwd.kernel", (256, 512))
    assert R.block_specs(40, {"units": 128, "bidirectional": False}, "rnn0") == [("rnn0.kernel", (40, 384)), ("rnn0.recurrent_kernel", (128, 384)),
                                                                                 ("rnn0.bias", (2, 384))]


# ---------------------------------------------------------------- the C ABI
def test_header_binding_and_library_agree_on_the_new_symbols(seld_lib):
    from seld_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "seld_hip.h")).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, f"include/seld_hip.h does not declare {name}"
        params = [p.strip() for p in m.group(1).split(",")]
        res, args = _lib.SIGNATURES[name]
        assert res is _lib._I and len(args) == len(params), name
        for p, a in zip(params, args):
            want = _lib._P if "*" in p else (_lib._L if p.startswith("int64_t") else _lib._I)
            assert a is want, f"{name}: {p!r} is bound as {a}"
        assert hasattr(seld_lib, name), f"libseld_hip.so does not export {name}"
    for mode, v in _lib.SELD_MERGE.items():
        assert re.search(r"#define SELD_MERGE_%s %d\b" % (mode.upper(), v), hdr)


# ---------------------------------------------------------------- fp32 against fp64 on the GPU cases
def _margin(name, a32, a64):
    e = rel_err(a32, a64)
    assert e <= FP32_MARGIN, f"{name}: fp32 is {e:.2e} from fp64"


@pytest.mark.parametrize("B,S,scale", [(b, s, 1.0) for b, s in R.LSTM_CASES + [R.UNI_CASE]] + [R.SATURATED])
def test_fp32_margin_of_the_lstm_cases(B, S, scale):
    ins = R.recurrence_inputs("lstm", B, S, scale)
    a, b = R.lstm_reference(ins, torch.float32), R.lstm_reference(ins)
    for k in ("h", "c", "dgx"):
        for d in (0, 1):
            _margin(f"lstm {(B, S, scale)} {k}[{d}]", a[k][d], b[k][d])


@pytest.mark.parametrize("B,S", R.GRU_DH_CASES + [R.GRU_MUL_CASE, R.UNI_CASE])
def test_fp32_margin_of_the_gru_cases(B, S):
    ins = R.recurrence_inputs("gru", B, S)
    a, b = R.gru_reference(ins, torch.float32), R.gru_reference(ins)
    for k in ("h", "dgx", "dgh"):
        for d in (0, 1):
            _margin(f"gru {(B, S)} {k}[{d}]", a[k][d], b[k][d])


@pytest.mark.parametrize("name", sorted(R.STAGE_CASES))
def test_fp32_margin_of_the_block_and_stage_cases(name):
    B, S, D, depth, cfg = R.STAGE_CASES[name]
    a, b = R.stage_reference(B, S, D, depth, cfg, 3, torch.float32), R.stage_reference(B, S, D, depth, cfg, 3)
    for k in ("out", "dx", "grad"):
        _margin(f"{name} {k}", a[k], b[k])
    off, biggest = 0, np.abs(b["grad"]).max()
    for n, s in b["specs"]:      # per variable, as the GPU test compares them
        kk = int(np.prod(s))
        if np.abs(b["grad"][off:off + kk]).max() >= 1e-9 * biggest:
            _margin(f"{name} grad {n}", a["grad"][off:off + kk], b["grad"][off:off + kk])
        off += kk


def test_fp32_margin_of_the_model_case(seldnet_config):
    from test_modules_gpu import STAGE_FIRST
    cfg = R.model_case(seldnet_config, STAGE_FIRST)
    B, T_ = R.MODEL_INPUT[:2]
    w, st = R.random_weights(cfg, R.MODEL_INPUT, seed=11)
    x, ys, yd = O.synthetic_batch(B, T_, seed=23)
    nthreads = torch.get_num_threads()
    torch.set_num_threads(1)      # the FIRST block's fp32 convolution gradients are not reliable under torch's CPU thread pool on every host
    try:
        b = R.train_step(cfg, R.MODEL_INPUT, w, st, x, ys, yd)
        a = R.train_step(cfg, R.MODEL_INPUT, w, st, x, ys, yd, dtype=torch.float32)
    finally:
        torch.set_num_threads(nthreads)
    for k in ("sed", "doa", "sloss", "dloss", "grad"):
        _margin(f"model {k}", a[k], b[k])
