"""CPU checks of the recurrent kinds under dropout / recurrent_dropout (tests/rnn_dropout_oracle.py): the identities that pin the LSTM
restatement, fp32 step loops with one planted fault each that the GPU tests' comparison must reject, the configuration rules of
seld_amd.modules.check_rnn_config / check_gru_config with dropout=True, the draw streams of a device-free build, the C ABI of the five new
operators, and — the margin under tests/test_rnn_dropout_gpu.py's 1e-4 bar — a plain fp32 evaluation of every GPU case within
tests/test_rnn_cpu.py's FP32_MARGIN of fp64."""
import copy
import os
import re

import numpy as np
import pytest
import torch

import rnn_dropout_oracle as RD
import rnn_oracle as R
from conftest import ROOT
from helpers import check, rel_err
from oracle import seldnet_oracle as O
from test_rnn_cpu import FP32_MARGIN, _as_kernel_outputs, _margin

NEW_SYMBOLS = ("seld_rnn_lstm_drop_fwd", "seld_rnn_lstm_drop_bwd", "seld_rnn_gru_drop_fwd", "seld_rnn_gru_drop_bwd", "seld_rnn_mask_rows")
LSTM_MARGIN_CASES = sorted(set(RD.LSTM_DROP_CASES + [R.UNI_CASE, RD.LSTM_BATCH_CASE, RD.LSTM_SMALLER_BATCH[:2]]))


# ---------------------------------------------------------------- identities that pin the restatement
@pytest.mark.parametrize("rate", RD.LSTM_RATES)
def test_masked_lstm_equals_the_unmasked_one_with_scaled_recurrent_rows(rate):
    """(h rm) U = h (diag(rm) U): clip by clip, the masked recurrence is the unmasked rnn_oracle one run with that clip's diag(rm_b) U — the
    form the kernels compute; without a mask it is rnn_oracle's"""
    B, S = 3, 17
    ins, masks = R.recurrence_inputs("lstm", B, S), R.gru_drop_masks(B, rate)
    assert (masks == 0).any(-1).all() and (masks > 1).any(-1).all()
    ref = RD.lstm_reference(ins, masks)
    plain, mine = R.lstm_reference(ins), RD.lstm_reference(ins)
    for d in (0, 1):
        for k in ("h", "c", "dgx"):
            assert np.array_equal(plain[k][d], mine[k][d])
        assert rel_err(ref["h"][d], plain["h"][d]) > 1e-2      # the mask matters
        for b in range(B):
            one = {"gx": ins["gx"][:, b:b + 1], "U": ins["U"].astype(np.float64) * masks[:, b, :, None].astype(np.float64), "dh": ins["dh"][:, b:b + 1]}
            alone = R.lstm_reference(one, dirs=(d,))
            for k in ("h", "c", "dgx"):
                assert rel_err(alone[k][0][0], ref[k][d][b]) <= 1e-12, (k, d, b)


def test_masked_lstm_recurrent_kernel_gradient_reads_the_masked_state():
    """dU = (h_prev * rm)^T dgx, which the blocks form from a mask-rows pass over h and the shifted product"""
    B, S = 3, 17
    ins, masks = R.recurrence_inputs("lstm", B, S), R.gru_drop_masks(B, 0.5)
    ref = RD.lstm_reference(ins, masks, with_dU=True)
    for d in (0, 1):
        hp = RD.shifted(ref["h"][d], d) * masks[d][:, None, :].astype(np.float64)
        assert rel_err(np.einsum("bsu,bsg->ug", hp, ref["dgx"][d]), ref["dU"][d]) <= 1e-12
        assert rel_err(np.einsum("bsu,bsg->ug", RD.shifted(ref["h"][d], d), ref["dgx"][d]), ref["dU"][d]) > 1e-2


def test_masked_lstm_direction_masks_the_input_ahead_of_the_projection():
    torch.manual_seed(3)
    B, S, D, u = 2, 5, 8, 128
    x = torch.randn(B, S, D, dtype=torch.float64)
    k, r, b = torch.randn(D, 4 * u, dtype=torch.float64), torch.randn(u, 4 * u, dtype=torch.float64) / u ** 0.5, torch.randn(4 * u, dtype=torch.float64)
    im = torch.tensor(R.gru_drop_masks(B, 0.5)[0][:, :D], dtype=torch.float64)
    a = RD.lstm_direction(x, k, r, b, False, in_mask=im)
    assert torch.equal(a, RD.lstm_direction(x * im[:, None, :], k, r, b, False))
    assert torch.equal(RD.lstm_direction(x, k, r, b, True), R.lstm_direction(x, k, r, b, True))


# ---------------------------------------------------------------- planted faults
def _lstm_fp32(ins, d, mask, fault=None):
    """a plain numpy fp32 step loop and BPTT of one direction under the state mask -> (h, c, saved [B,S,128,4], dgx), with one deliberate mistake
    of the kind a kernel could make: 'h': the mask is applied to the emitted h; 'c': the mask is applied to the cell state as well; 'carry': the
    gradient carried to the previous step is left unmasked; 'row': clip b uses clip b + 1's mask row"""
    f = np.float32
    gx, U, dh = ins["gx"][d], ins["U"][d], ins["dh"][d]
    m = np.roll(mask[d], -1, axis=0) if fault == "row" else mask[d]
    B, S, _ = gx.shape
    u = 128
    sig = lambda a: (1 / (1 + np.exp(-a, dtype=f))).astype(f)
    hs, cs, sv = np.zeros((B, S, u), f), np.zeros((B, S, u), f), np.zeros((B, S, u, 4), f)
    h, c = np.zeros((B, u), f), np.zeros((B, u), f)
    order = list(range(S - 1, -1, -1) if d else range(S))
    for t in order:
        z = gx[:, t] + (h * m) @ U
        i, fg, g, o = sig(z[:, :u]), sig(z[:, u:2 * u]), np.tanh(z[:, 2 * u:3 * u]), sig(z[:, 3 * u:])
        c = fg * (c * m if fault == "c" else c) + i * g
        h = o * np.tanh(c)
        hs[:, t], cs[:, t], sv[:, t] = (h * m if fault == "h" else h), c, np.stack([i, fg, g, o], -1)
    dgx = np.zeros((B, S, 4 * u), f)
    carry, dcc = np.zeros((B, u), f), np.zeros((B, u), f)
    for n in range(S - 1, -1, -1):
        t = order[n]
        cprev = cs[:, order[n - 1]] if n > 0 else np.zeros((B, u), f)
        i, fg, g, o = (sv[:, t, :, k] for k in range(4))
        tc = np.tanh(cs[:, t])
        g_h = dh[:, t] + carry
        dc = g_h * o * (1 - tc * tc) + dcc
        dz = np.concatenate([dc * g * i * (1 - i), dc * cprev * fg * (1 - fg), dc * i * (1 - g * g), g_h * tc * o * (1 - o)], -1)
        dcc = dc * fg
        dgx[:, t] = dz
        carry = dz @ U.T if fault == "carry" else (dz @ U.T) * m
        assert carry.dtype == f
    return hs, cs, sv, dgx


def _lstm_compare(tag, got, ref, d, tol=1e-4):
    """the GPU test's comparison of one direction: helpers.check on h, c, saved and dgx -> {name: error}; raises for the first beyond tol"""
    errs = {k: rel_err(a, ref[k][d]) for k, a in zip(("h", "c", "saved", "dgx"), got)}
    for k, a in zip(("h", "c", "saved", "dgx"), got):
        check(f"{tag} {k}[{d}]", a, ref[k][d], tol)
    return errs


@pytest.mark.parametrize("fault", [None, "h", "c", "carry", "row"])
def test_the_lstm_comparison_can_fail(fault):
    """the comparison tests/test_rnn_dropout_gpu.py holds the kernels to passes a correct fp32 evaluation and reports each wrong one above 1e-4"""
    B, S = 3, 17
    ins, masks = R.recurrence_inputs("lstm", B, S), R.gru_drop_masks(B, 0.5)
    ref = RD.lstm_reference(ins, masks)
    for d in (0, 1):
        got = _lstm_fp32(ins, d, masks, fault)
        if fault is None:
            assert max(_lstm_compare("fp32 step loop", got, ref, d).values()) <= FP32_MARGIN
            continue
        with pytest.raises(AssertionError, match="rel err"):
            _lstm_compare(f"{fault}[{d}]", got, ref, d)
        errs = {k: rel_err(a, ref[k][d]) for k, a in zip(("h", "c", "saved", "dgx"), got)}
        if fault == "h":          # the state is right, what is emitted is not
            assert errs["c"] <= FP32_MARGIN and errs["h"] > 1e-4
        elif fault == "carry":    # the forward is right
            assert max(errs[k] for k in ("h", "c", "saved")) <= FP32_MARGIN and errs["dgx"] > 1e-4
        else:
            assert errs["h"] > 1e-4 and errs["c"] > 1e-4 and errs["dgx"] > 1e-4


# ---------------------------------------------------------------- configuration rules
def test_dropout_keyword_accepts_any_rate_below_one():
    from seld_amd import modules
    for rate in (0.0, 0.3, 0.999, None):
        modules.check_rnn_config({"units": 128, "dropout_rate": rate}, dropout=True)
        modules.check_rnn_config({"units": 128, "depth": 2, "dropout_rate": rate}, True, dropout=True)
        modules.check_gru_config({"units": [128, 128], "dropout_rate": rate}, dropout=True)
    modules.check_rnn_config({"units": 128}, dropout=True)
    modules.check_gru_config({"units": [128]}, dropout=True)
    for rate in (1.0, -0.1, float("nan"), 1.5):
        with pytest.raises(ValueError, match="dropout_rate"):
            modules.check_rnn_config({"units": 128, "dropout_rate": rate}, dropout=True)
        with pytest.raises(ValueError, match="dropout_rate"):
            modules.check_gru_config({"units": [128], "dropout_rate": rate}, dropout=True)
    # every other rule holds under the keyword
    with pytest.raises(ValueError, match="128 units"):
        modules.check_rnn_config({"units": 64, "dropout_rate": 0.3}, dropout=True)
    with pytest.raises(ValueError, match="128 units"):
        modules.check_gru_config({"units": [128, 64], "dropout_rate": 0.3}, dropout=True)
    with pytest.raises(ValueError, match="merge_mode"):
        modules.check_rnn_config({"units": 128, "merge_mode": "avg", "dropout_rate": 0.3}, dropout=True)
    # without it both refuse as before
    with pytest.raises(ValueError, match="not implemented on the composed path"):
        modules.check_rnn_config({"units": 128, "dropout_rate": 0.3})
    with pytest.raises(ValueError, match="exist on the fused path only"):
        modules.check_gru_config({"units": [128], "dropout_rate": 0.3})


def test_the_references_test_configs_are_accepted_as_written_at_128_units():
    """modules_test.py:32-59, 226-242 with units 128 and their own dropout_rate 0.3, through the route the models take"""
    from seld_amd import modules
    assert set(modules.RNN_SECOND + ("bidirectional_GRU_block",)) <= set(modules.DROPOUT_KINDS)
    for cfg, stage in R.REFERENCE_CONFIGS:
        c = dict(copy.deepcopy(cfg), units=128)
        kind = "RNN_stage" if stage else "RNN_block"
        modules._check_second(kind, c, None, dropout=True)
        if c["dropout_rate"]:
            with pytest.raises(ValueError, match="dropout"):
                modules._check_second(kind, c, None)
            with pytest.raises(ValueError, match="dropout"):      # the stand-alone factories keep their refusal
                (modules.RNN_stage if stage else modules.RNN_block)(c)
    modules._check_second("bidirectional_GRU_block", {"units": [128, 128], "dropout_rate": 0.3}, None, dropout=True)


def test_a_device_free_build_gives_each_block_its_draw_streams(seld_lib):
    from seld_amd import modules
    rt = modules._Rt(torch.device("meta"))
    rt.dropout = True
    B, S, D = 2, 12, 40
    st = modules._build_second("RNN_stage", rt, {"units": 128, "depth": 3, "rnn_type": "LSTM", "merge_mode": "concat", "dropout_rate": 0.3}, S, D, B)
    assert [b.drop.base for b in st.blocks] == [4096, 4128, 4160] and all(b.drop.rate == float(np.float32(0.3)) for b in st.blocks)
    assert [b.D for b in st.blocks] == [40, 256, 256] and st.blocks[1].im[1].shape == (B, 256) and st.blocks[1].rm[1].shape == (B, 128)
    g = modules._build_second("bidirectional_GRU_block", rt, {"units": [128, 128], "dropout_rate": 0.2}, S, D, B, prefix="doa.gru", first_block=5)
    assert [b.drop.base for b in g.blocks] == [4096 + 32 * 5, 4096 + 32 * 6] and g.blocks[0].dh is not None
    one = modules._build_second("RNN_block", rt, {"units": 128, "bidirectional": False, "dropout_rate": 0.2}, S, D, B, prefix="u", first_block=9)
    assert one.blocks[0].drop.base == 4096 + 32 * 9 and len(one.blocks[0].im) == 1
    # rate 0: no mask buffers, and a width the mask kernel cannot move is refused at construction only where masks are drawn
    off = modules._build_second("RNN_block", rt, {"units": 128, "dropout_rate": 0.0}, S, 42, B, prefix="z")
    assert off.blocks[0].drop.rate == 0.0 and not hasattr(off.blocks[0], "im")
    with pytest.raises(ValueError, match="D % 4"):
        modules._build_second("RNN_block", rt, {"units": 128, "dropout_rate": 0.2}, S, 42, B, prefix="y")


def test_conv_temporal_on_ss5_builds_with_a_recurrent_dropout_rate(seld_lib):
    """SS5.json's DOA head is a bidirectional_GRU_stage without a dropout_rate; with a rate set by the caller its blocks own masks on their own streams"""
    import json
    from seld_amd import modules
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "SS5.json")))
    assert cfg["DOA"] == "bidirectional_GRU_stage" and not cfg["DOA_ARGS"].get("dropout_rate")
    plain = modules.ConvTemporalNet((1, 300, 64, 7), cfg, "meta")
    assert all(b.drop.rate == 0.0 and not hasattr(b, "im") for b in plain.heads[1].body.blocks)
    cfg["DOA_ARGS"]["dropout_rate"] = 0.3
    m = modules.ConvTemporalNet((1, 300, 64, 7), cfg, "meta")
    blocks = m.heads[1].body.blocks
    assert blocks and all(type(b).__name__ == "BidirectionalGRUBlock" and b.drop.rate == float(np.float32(0.3)) for b in blocks)
    assert [b.drop.base for b in blocks] == [m.stream_bases["doa.gru"] + 32 * i for i in range(len(blocks))]
    assert all(b.im[1].shape == (1, b.D) and b.rm[0].shape == (1, 128) and b.dh is not None for b in blocks)
    assert [(n, s) for n, _, s in m.variables] == [(n, s) for n, _, s in plain.variables]


def test_oracle_masks_are_the_librarys_draws():
    """cell_masks: element e of the row-major mask is uniform e of stream 4096 + 32 index + site — seld_dropout applied to ones"""
    B, D, rate = 3, 40, 0.3
    for index, d in ((0, 0), (2, 1)):
        im, rm = RD.cell_masks(B, D, rate, index, 7, d)
        for site, m, width in ((2 * d, im, D), (2 * d + 1, rm, 128)):
            u = O.philox_uniform(B * width, RD.DO.SEED, 4096 + 32 * index + site, 7).reshape(B, width)
            want = (u >= np.float32(rate)) / (1.0 - float(np.float32(rate)))
            assert np.array_equal(m.numpy(), want) and 0 < (m == 0).double().mean() < 1


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
        assert params[-1] == "void* stream", name


# ---------------------------------------------------------------- fp32 against fp64 on the GPU cases
@pytest.mark.parametrize("rate", RD.LSTM_RATES)
@pytest.mark.parametrize("B,S", LSTM_MARGIN_CASES)
def test_fp32_margin_of_the_lstm_dropout_cases(B, S, rate):
    ins, masks = R.recurrence_inputs("lstm", B, S), R.gru_drop_masks(B, rate)
    a, b = RD.lstm_reference(ins, masks, torch.float32), RD.lstm_reference(ins, masks)
    for k in ("h", "c", "saved", "dgx"):
        for d in (0, 1):
            _margin(f"lstm dropout {(B, S, rate)} {k}[{d}]", a[k][d], b[k][d])
    assert max(np.abs(c).max() for c in b["c"]) <= 4


@pytest.mark.parametrize("B,S", sorted(set(R.GRU_DROP_CASES + R.GRU_DROP_AT_CHUNKS + [R.UNI_CASE])))
def test_fp32_margin_of_the_gru_dropout_cases_per_direction(B, S):
    """the directions' output gradients as given (test_rnn_cpu.py holds the 'mul'-merged form of the same cases)"""
    ins, masks = R.recurrence_inputs("gru", B, S), R.gru_drop_masks(B, R.GRU_DROP_RATE)
    a, b = R.gru_reference(ins, torch.float32, rec_mask=masks), R.gru_reference(ins, rec_mask=masks)
    R.gru_compare(f"gru dropout dh {(B, S)}", _as_kernel_outputs(a), b, FP32_MARGIN)


@pytest.mark.parametrize("name", sorted(RD.STAGE_CASES))
def test_fp32_margin_of_the_block_and_stage_cases(name):
    kind, B, S, D, cfg = RD.STAGE_CASES[name]
    for step in (0, 1):
        a = RD.stage_reference(kind, B, S, D, cfg, RD.STAGE_SEED, step, torch.float32)
        b = RD.stage_reference(kind, B, S, D, cfg, RD.STAGE_SEED, step)
        for k in ("out", "dx", "grad"):
            _margin(f"{name} step {step} {k}", a[k], b[k])
        off, biggest = 0, np.abs(b["grad"]).max()
        for n, s in b["specs"]:      # per variable, as the GPU test compares them
            kk = int(np.prod(s))
            if np.abs(b["grad"][off:off + kk]).max() >= 1e-9 * biggest:
                _margin(f"{name} grad {n}", a["grad"][off:off + kk], b["grad"][off:off + kk])
            off += kk
    plain = RD.stage_reference(kind, B, S, D, cfg, RD.STAGE_SEED, None)
    assert rel_err(b["out"], plain["out"]) > 1e-2      # the masks matter


def test_inference_of_the_oracle_is_rnn_oracles(seldnet_config):
    kind, B, S, D, cfg = RD.STAGE_CASES["lstm stage depth 2 concat"]
    a = RD.stage_reference(kind, B, S, D, cfg, RD.STAGE_SEED, None)
    b = R.stage_reference(B, S, D, 2, dict(cfg, dropout_rate=0.0), RD.STAGE_SEED)
    for k in ("out", "dx", "grad"):
        assert np.array_equal(a[k], b[k])


def test_fp32_margin_of_the_model_case(seldnet_config):
    from test_modules_gpu import STAGE_FIRST
    cfg = RD.model_case(seldnet_config, STAGE_FIRST)
    B, T_ = R.MODEL_INPUT[:2]
    w, st = R.random_weights(cfg, R.MODEL_INPUT, seed=11)
    x, ys, yd = O.synthetic_batch(B, T_, seed=23)
    nthreads = torch.get_num_threads()
    torch.set_num_threads(1)      # as tests/test_rnn_cpu.py's model case
    try:
        b = RD.train_step(cfg, R.MODEL_INPUT, w, st, x, ys, yd, dropout_step=0)
        a = RD.train_step(cfg, R.MODEL_INPUT, w, st, x, ys, yd, dropout_step=0, dtype=torch.float32)
    finally:
        torch.set_num_threads(nthreads)
    for k in ("sed", "doa", "sloss", "dloss", "grad"):
        _margin(f"model {k}", a[k], b[k])
    plain = R.train_step(cfg, R.MODEL_INPUT, w, st, x, ys, yd)
    assert rel_err(b["grad"], plain["grad"]) > 1e-2
