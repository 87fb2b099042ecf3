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

NEW_SYMBOLS = ("seld_rnn_lstm_fwd", "seld_rnn_lstm_bwd", "seld_rnn_gru_fwd", "seld_rnn_gru_bwd", "seld_rnn_merge_fwd", "seld_rnn_merge_bwd",
               "seld_k_gru_drop_fwd", "seld_k_gru_drop_bwd")
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


def test_masked_gru_recurrence_matches_the_oracle_gru_direction():
    """recurrent dropout: R.gru_recurrence(rec_mask=...) against oracle.seldnet_oracle.gru_direction(rec_mask=...), the restatement of Keras
    GRUCell.call that the model tests run on; and what it hands out as the saved gates rebuilds h from the MASKED previous state"""
    torch.manual_seed(2)
    B, S, D, u = 3, 9, 20, 128
    x = torch.randn(B, S, D, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(B, S, u, dtype=torch.float64)
    k, r, b = torch.randn(D, 3 * u, dtype=torch.float64) / D ** 0.5, torch.randn(u, 3 * u, dtype=torch.float64) / u ** 0.5, 0.1 * torch.randn(2, 3 * u, dtype=torch.float64)
    m = torch.tensor(R.gru_drop_masks(B, 0.5)[0], dtype=torch.float64)
    assert 0.2 < float((m == 0).double().mean()) < 0.8
    for rev in (False, True):
        want = O.gru_direction(x, k, r, b, rev, rec_mask=m)
        aux = {}
        mine = R.gru_recurrence(x @ k + b[0], r, b[1], rev, rec_mask=m, aux=aux)
        (gw,), (gm,) = torch.autograd.grad((want * dy).sum(), x), torch.autograd.grad((mine * dy).sum(), x)
        assert rel_err(mine.detach().numpy(), want.detach().numpy()) <= 1e-10
        assert rel_err(gm.numpy(), gw.numpy()) <= 1e-10
        assert rel_err(mine.detach().numpy(), O.gru_direction(x, k, r, b, rev).detach().numpy()) > 1e-2      # the mask matters
        h = mine.detach()
        hp = torch.zeros_like(h)      # the masked previous state
        if rev:
            hp[:, :-1] = h[:, 1:] * m[:, None, :]
        else:
            hp[:, 1:] = h[:, :-1] * m[:, None, :]
        assert rel_err((aux["z"] * hp + (1 - aux["z"]) * aux["hh"]).numpy(), h.numpy()) <= 1e-12
        assert rel_err(aux["gh_h"].numpy(), (hp @ r + b[1])[..., 2 * u:].numpy()) <= 1e-12
        assert rel_err(aux["hh"].numpy(), torch.tanh((x @ k + b[0])[..., 2 * u:] + aux["r"] * aux["gh_h"]).detach().numpy()) <= 1e-12


def _gru_steps_fp32(ins, d, mask=None, fault=None):
    """a plain numpy fp32 step loop of one direction -> (h, hm, saved [B,S,128,4]), with one deliberate mistake of the kind a kernel could make:
    'border': h_prev is taken from the wrong neighbour at ONE step, the first of the forward kernel's second chunk (t = 16 in the forward
    direction, t = S - 17 in the reverse one); 'swap': z and r change places in the saved gates; 'blend': the blend uses the unmasked state"""
    gx, U, brec = ins["gx"][d], ins["U"][d], ins["brec"][d]
    B, S, _ = gx.shape
    u = 128
    sig = lambda a: (1 / (1 + np.exp(-a, dtype=np.float32))).astype(np.float32)
    hs, sv = np.zeros((B, S, u), np.float32), np.zeros((B, S, u, 4), np.float32)
    h = np.zeros((B, u), np.float32)
    order = list(range(S - 1, -1, -1) if d else range(S))
    for n, t in enumerate(order):
        raw = h
        if fault == "border" and n == 16:
            raw = hs[:, order[n - 2]]
        hp = raw if mask is None else raw * mask[d]
        gh = hp @ U + brec
        z, r = sig(gx[:, t, :u] + gh[:, :u]), sig(gx[:, t, u:2 * u] + gh[:, u:2 * u])
        hh = np.tanh(gx[:, t, 2 * u:] + r * gh[:, 2 * u:])
        h = z * (raw if fault == "blend" else hp) + (1 - z) * hh
        hs[:, t] = h
        sv[:, t] = np.stack([r, z, hh, gh[:, 2 * u:]] if fault == "swap" else [z, r, hh, gh[:, 2 * u:]], -1)
    return hs, (hs if mask is None else hs * mask[d][:, None, :]), sv


@pytest.mark.parametrize("fault", [None, "border", "swap", "blend"])
def test_the_gru_comparison_can_fail(fault):
    """R.gru_compare, the function tests/test_gru_gpu.py holds the kernels to, passes a correct fp32 evaluation and reports each wrong one above the
    GPU tests' 1e-4"""
    B, S = 3, 33
    ins = R.recurrence_inputs("gru", B, S)
    masks = R.gru_drop_masks(B, R.GRU_DROP_RATE) if fault == "blend" else None
    ref = R.gru_reference(ins, rec_mask=masks)
    if fault is None:
        R.gru_compare("fp32 oracle", _as_kernel_outputs(R.gru_reference(ins, torch.float32)), ref, 1e-4)
        masks = R.gru_drop_masks(B, R.GRU_DROP_RATE)
        ref_m = R.gru_reference(ins, rec_mask=masks)
        R.gru_compare("fp32 oracle, masked", _as_kernel_outputs(R.gru_reference(ins, torch.float32, rec_mask=masks)), ref_m, 1e-4)
        for m, rf in ((None, ref), (masks, ref_m)):      # the step loop that carries the mistakes below is right without them
            runs = [_gru_steps_fp32(ins, d, m) for d in (0, 1)]
            got = {"h": [x[0] for x in runs], "saved": [x[2] for x in runs]}
            if m is not None:
                got["hm"] = [x[1] for x in runs]
            R.gru_compare("fp32 step loop", got, rf, 1e-4)
        return
    for d in (0, 1):
        h, hm, sv = _gru_steps_fp32(ins, d, masks, fault)
        got = {"h": [h], "saved": [sv]}
        one = {k: [v[d]] for k, v in ref.items()}
        with pytest.raises(AssertionError, match="rel err"):
            R.gru_compare(f"{fault}[{d}]", got, one, 1e-4)
        errs = {n: rel_err(a, b) for n, a, b in R.gru_pieces(got, one)}
        if fault == "swap":      # h is right; the two planes alone are wrong
            assert errs["h[0]"] <= FP32_MARGIN and errs["saved[0].z"] > 1e-4 and errs["saved[0].r"] > 1e-4 and errs["saved[0].hh"] <= FP32_MARGIN
        else:
            assert errs["h[0]"] > 1e-4, errs
        if fault == "border":      # one step alone is wrong, and what follows it
            t = 16 if d == 0 else S - 17
            before = slice(0, t) if d == 0 else slice(t + 1, S)
            assert rel_err(h[:, before], ref["h"][d][:, before]) <= FP32_MARGIN and rel_err(h[:, t], ref["h"][d][:, t]) > 1e-4


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


# ---------------------------------------------------------------- refusal order of the eight 128-unit recurrences, without a device
# REFUSED calls only: each returns before any HIP call, so nothing is dereferenced and no device is needed.  The rules, in order:
#   1. units != 128 -> UNSUPPORTED;  2. a required pointer NULL, B or S < 1 -> INVALID;  3. half a second direction -> INVALID;
#   4. S > 2^20 or B > 0x3fffffff -> UNSUPPORTED.
# The plain forwards may leave `saved` (the LSTM: and `c`) NULL, but for every direction alike; the DROP forms require them.
INVALID, UNSUPPORTED = -1, -2
_pairs = lambda *stems: [f"{s}_{d}" for s in stems for d in "fb"]
RNN_ENTRIES = {      # entry -> (argument names in call order, the *_f arguments that may be NULL)
    "seld_rnn_lstm_fwd": (_pairs("gx", "U", "h", "c", "saved"), {"c_f", "saved_f"}),
    "seld_rnn_lstm_bwd": (_pairs("dh", "c", "saved", "U", "dgx"), set()),
    "seld_rnn_gru_fwd": (_pairs("gx", "U", "brec", "h", "saved"), {"saved_f"}),
    "seld_rnn_gru_bwd": (_pairs("dh", "h", "saved", "U", "dgx", "dgh"), set()),
    "seld_rnn_lstm_drop_fwd": (_pairs("gx", "U", "rm", "h", "c", "saved"), set()),
    "seld_rnn_lstm_drop_bwd": (_pairs("dh", "c", "saved", "U", "rm", "dgx"), set()),
    "seld_rnn_gru_drop_fwd": (_pairs("gx", "U", "brec", "rm", "h", "hm", "saved"), set()),
    "seld_rnn_gru_drop_bwd": (_pairs("dh", "hm", "saved", "U", "rm", "dgx", "dgh"), set()),
}


@pytest.mark.parametrize("op", sorted(RNN_ENTRIES))
def test_refusal_order_of_the_128_unit_entries(seld_lib, op):
    import ctypes as C
    names, optional = RNN_ENTRIES[op]
    p = C.c_void_p(1 << 20)      # never dereferenced: every call below is refused first

    def call(B=1, S=1, units=128, **over):
        return getattr(seld_lib, op)(*[over.get(n, p) for n in names], B, S, units, None)

    one = {n: None for n in names if n.endswith("_b")}      # one direction
    req = [n for n in names if n.endswith("_f") and n not in optional]
    for u in (0, 127, 129):      # the width first, whatever else is wrong
        assert call(units=u) == UNSUPPORTED
        assert call(units=u, **{req[0]: None}) == UNSUPPORTED
        assert call(units=u, B=0) == UNSUPPORTED
    for n in req:      # each required pointer, with two directions and with one
        assert call(**{n: None}) == INVALID, n
        assert call(**one, **{n: None}) == INVALID, n
        assert call(S=(1 << 20) + 1, **{n: None}) == INVALID, n      # the pointer before the length
    for bad in ({"B": 0}, {"B": -1}, {"S": 0}, {"S": -1}):
        assert call(**bad) == INVALID, bad
        assert call(**one, **bad) == INVALID, bad
    for n in one:      # half a second direction: one *_b argument missing, and one *_b argument alone
        assert call(**{n: None}) == INVALID, n
        if n != names[1]:      # names[1] (gx_b / dh_b) decides how many directions there are
            assert call(**{m: None for m in one if m != n}) == INVALID, n
        assert call(S=(1 << 20) + 1, **{n: None}) == INVALID, n
    for n in sorted(optional):      # a plain forward: saved (and c) for one direction only, or saved without c
        assert call(**{n: None}) == INVALID, n
        assert call(**{n[:-1] + "b": None}) == INVALID, n
        if len(optional) == 2:
            assert call(**one, **{n: None}) == INVALID, n
    if "drop" in op:      # the DROP forms always save
        assert call(saved_f=None) == INVALID and call(saved_f=None, saved_b=None) == INVALID
        assert call(**one, saved_f=None) == INVALID
    for kw in ({}, one):
        assert call(S=(1 << 20) + 1, **kw) == UNSUPPORTED
        assert call(B=(1 << 30), **kw) == UNSUPPORTED
        assert call(B=(1 << 30), S=(1 << 20) + 1, **kw) == UNSUPPORTED


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


def _as_kernel_outputs(ref):
    """a gru_reference result in the shape the GPU tests hand to R.gru_compare: the four saved quantities as one [B,S,128,4] tensor per direction"""
    got = {k: v for k, v in ref.items() if k not in R.GRU_SAVED}
    got["saved"] = [R.gru_saved(ref, i) for i in range(len(ref["h"]))]
    return got


def _gru_margin(tag, ins, **kw):
    """fp32 against fp64 through the GPU tests' own comparison (per direction, per gate block) at FP32_MARGIN; -> the fp64 result"""
    a, b = R.gru_reference(ins, torch.float32, **kw), R.gru_reference(ins, **kw)
    R.gru_compare(tag, _as_kernel_outputs(a), b, FP32_MARGIN)
    return b


GRU_PLAIN_CASES = sorted(set(R.GRU_DH_CASES + [R.GRU_MUL_CASE, R.UNI_CASE, R.GRU_BATCH_CASE, R.GRU_SMALLER_BATCH[:2]] + R.GRU_EDGE_CASES))


@pytest.mark.parametrize("B,S", GRU_PLAIN_CASES)
def test_fp32_margin_of_the_gru_cases(B, S):
    """every (B, S) of tests/test_rnn_gpu.py and tests/test_gru_gpu.py without dropout, with the directions' output gradients as given and with the
    'mul' merge's: h, out, the saved gates, dgx, dgh"""
    ins = R.recurrence_inputs("gru", B, S)
    a, b = R.gru_reference(ins, torch.float32), _gru_margin(f"gru dh {(B, S)}", ins)
    for k in ("h", "dgx", "dgh"):
        for d in (0, 1):
            _margin(f"gru {(B, S)} {k}[{d}]", a[k][d], b[k][d])
    _gru_margin(f"gru mul {(B, S)}", ins, mul=True)


def test_fp32_margin_of_the_saturated_gru_case():
    B, S, scale = R.GRU_SATURATED
    ins = R.recurrence_inputs("gru", B, S, scale)
    assert np.abs(ins["gx"]).max() > 30
    _gru_margin(f"gru dh x{scale}", ins)
    _gru_margin(f"gru mul x{scale}", ins, mul=True)


@pytest.mark.parametrize("B,S", sorted(set(R.GRU_DROP_CASES + R.GRU_DROP_AT_CHUNKS + R.GRU_DROP_BPTT_CASES + [R.GRU_BATCH_CASE])))
def test_fp32_margin_of_the_gru_dropout_cases(B, S):
    """Keras scales the masked state by 1 / (1 - rate) at every step, so |h| is not bounded by 1 under recurrent dropout: the rate and the lengths
    of the cases are those at which the state stays small (|h| <= 4 in fp64) and fp32 stays within the margin"""
    ins, masks = R.recurrence_inputs("gru", B, S), R.gru_drop_masks(B, R.GRU_DROP_RATE)
    assert set(np.unique(masks)) == {0.0, np.float32(1 / (1 - R.GRU_DROP_RATE))} and (masks == 0).any(-1).all()      # every clip drops a unit
    b = _gru_margin(f"gru dropout {(B, S)}", ins, rec_mask=masks, mul=True)
    assert max(np.abs(h).max() for h in b["h"]) <= 4
    for d in (0, 1):
        assert np.array_equal(b["hm"][d], b["h"][d] * masks[d][:, None, :].astype(np.float64))


def _bptt_fp32(ref, ins, d, dh, mask=None):
    """the backward pass alone, as tests/test_gru_gpu.py's isolated test feeds the kernels: a plain numpy fp32 BPTT of direction d (the equations at
    the head of gru.hip's backward kernel) on the fp64 oracle's h, hm and saved quantities rounded to fp32 -> dgx, dgh [B,S,384]"""
    f = np.float32
    z, r, hh, gh = (R.f32(ref[k][d]) for k in R.GRU_SAVED)
    hprev_src = R.f32(ref["hm" if mask is not None else "h"][d])
    U, dh = R.f32(ins["U"][d]), R.f32(dh)
    B, S, u = z.shape
    dgx, dgh = np.zeros((B, S, 3 * u), f), np.zeros((B, S, 3 * u), f)
    carry = np.zeros((B, u), f)
    for t in (range(S) if d else range(S - 1, -1, -1)):      # the forward's processing order, backwards
        tp = t + 1 if d else t - 1
        hp = hprev_src[:, tp] if 0 <= tp < S else np.zeros((B, u), f)
        g = dh[:, t] + carry
        a_h = g * (1 - z[:, t]) * (1 - hh[:, t] * hh[:, t])
        a_z = g * (hp - hh[:, t]) * z[:, t] * (1 - z[:, t])
        a_r = a_h * gh[:, t] * r[:, t] * (1 - r[:, t])
        dgx[:, t] = np.concatenate([a_z, a_r, a_h], -1)
        dgh[:, t] = np.concatenate([a_z, a_r, a_h * r[:, t]], -1)
        carry = g * z[:, t] + dgh[:, t] @ U.T
        if mask is not None:
            carry = carry * mask[d]
        assert carry.dtype == f
    return dgx, dgh


@pytest.mark.parametrize("S", R.GRU_BPTT_S)
def test_fp32_margin_of_the_isolated_bptt_cases(S):
    B = 2
    ins = R.recurrence_inputs("gru", B, S)
    ref = R.gru_reference(ins)
    runs = [_bptt_fp32(ref, ins, d, ins["dh"][d]) for d in (0, 1)]
    R.gru_compare(f"bptt dh {(B, S)}", {"dgx": [x[0] for x in runs], "dgh": [x[1] for x in runs]}, ref, FP32_MARGIN)
    ref = R.gru_reference(ins, mul=True)
    runs = [_bptt_fp32(ref, ins, d, ins["dh"][0] * R.f32(ref["h"][1 - d])) for d in (0, 1)]
    R.gru_compare(f"bptt mul {(B, S)}", {"dgx": [x[0] for x in runs], "dgh": [x[1] for x in runs]}, ref, FP32_MARGIN)
    B = R.GRU_DROP_BPTT_CASES[0][0]
    ins, masks = R.recurrence_inputs("gru", B, S), R.gru_drop_masks(B, R.GRU_DROP_RATE)
    ref = R.gru_reference(ins, rec_mask=masks, mul=True)
    runs = [_bptt_fp32(ref, ins, d, ins["dh"][0] * R.f32(ref["h"][1 - d]), masks) for d in (0, 1)]
    R.gru_compare(f"bptt drop {(B, S)}", {"dgx": [x[0] for x in runs], "dgh": [x[1] for x in runs]}, ref, FP32_MARGIN)


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
