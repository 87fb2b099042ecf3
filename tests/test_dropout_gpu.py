"""The composed path's Dropout on the device against tests/dropout_oracle.py: seld_dropout element by element,
seld_attn_drop_fwd / _bwd at the tile edges, the three attention blocks' training forward and backward through the modules.py factories, and one
train step of a composed model.  Mask decisions are integer compares of the same Philox words on both sides: helpers.REL_TOL as everywhere."""
import copy
import ctypes as C
import math

import numpy as np
import pytest
import torch

import attention_block_oracle as A
import conformer_oracle as CF
import dropout_oracle as DO
import transformer_oracle as T
from helpers import check, dev, ptr
from test_attention_gpu import _Window, _check_or_zero, _odd_strides, _stream

pytestmark = pytest.mark.gpu

SEED = DO.SEED


# ---------------------------------------------------------------- seld_dropout
def _m_dropout(lib, x, out, rate, alpha, accumulate, layer, step, seed=SEED):
    assert lib.seld_dropout(ptr(x), ptr(out), x.numel(), rate, alpha, accumulate, seed, layer, step, _stream()) == 0


def _within_one_ulp(name, got, want64):
    """got fp32 against the exact fp64 value: zeros are zeros, the rest within one unit in the last place of the fp32 result"""
    got = np.asarray(got, np.float32)
    assert np.array_equal(got == 0, want64 == 0), name
    ulp = np.spacing(np.abs(want64).astype(np.float32)).astype(np.float64)
    assert (np.abs(got.astype(np.float64) - want64) <= ulp).all(), name


@pytest.mark.parametrize("rate", [0.1, 0.5])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 4100])
def test_m_dropout_matches_the_oracle_draws(seld_lib, n, rate):
    from oracle import seldnet_oracle as O
    layer, step, alpha = 4096 + 32 * 3 + 5, 11, 0.75
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n).astype(np.float32)
    x[x == 0] = 1.0
    y0 = rng.standard_normal(n).astype(np.float32)
    mask = O.dropout_mask((n,), rate, SEED, layer, step, torch.float64).numpy()      # 0 | 1 / (1 - fp32 rate)
    assert 0 < (mask != 0).sum() or n < 8
    xd = dev(x)
    # a band behind the n elements stays untouched (the tail of the last group of four is not written)
    out = torch.full((n + 8,), float("nan"), device="cuda")
    _m_dropout(seld_lib, xd, out, rate, 1.0, 0, layer, step)
    _within_one_ulp("alpha 1", out[:n].cpu().numpy(), x.astype(np.float64) * mask)
    assert bool(torch.isnan(out[n:]).all())
    _m_dropout(seld_lib, xd, out, rate, alpha, 0, layer, step)
    _within_one_ulp("alpha", out[:n].cpu().numpy(), alpha * x.astype(np.float64) * mask)
    # accumulate: out += alpha in mask, one rounding
    acc = torch.full((n + 8,), float("nan"), device="cuda")
    acc[:n].copy_(dev(y0))
    _m_dropout(seld_lib, xd, acc, rate, alpha, 1, layer, step)
    want = y0.astype(np.float64) + alpha * x.astype(np.float64) * mask
    got = acc[:n].cpu().numpy()
    assert (np.abs(got - want) <= np.spacing(np.maximum(np.abs(want), np.abs(y0)).astype(np.float32))).all()
    assert np.array_equal(got[mask == 0], y0[mask == 0]) and bool(torch.isnan(acc[n:]).all())
    # in place (the backward's use on gradients), and twice the same bits
    inplace = dev(x)
    _m_dropout(seld_lib, inplace, inplace, rate, 1.0, 0, layer, step)
    _m_dropout(seld_lib, xd, out, rate, 1.0, 0, layer, step)
    assert torch.equal(inplace, out[:n])
    # another stream or step: other draws (n large enough to tell); rate 0: the identity
    if n >= 1023:
        for lay, stp in ((layer + 1, step), (layer, step + 1)):
            other = torch.empty(n, device="cuda")
            _m_dropout(seld_lib, xd, other, rate, 1.0, 0, lay, stp)
            assert not torch.equal(other, out[:n])
    ident = torch.full((n,), float("nan"), device="cuda")
    _m_dropout(seld_lib, xd, ident, 0.0, 1.0, 0, layer, step)
    assert torch.equal(ident, xd)


def test_entry_points_refuse_bad_arguments_on_the_device(seld_lib):
    from test_dropout_cpu import drop_entry_points_refuse_bad_arguments
    buf = torch.zeros(64, device="cuda")
    drop_entry_points_refuse_bad_arguments(seld_lib, ptr(buf))
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0      # nothing was enqueued


# ---------------------------------------------------------------- seld_attn_drop_fwd / _bwd
def _attn_drop(lib, q, k, v, do, B, S, H, d, scale, rate, layer, step, odd=False, seed=SEED, plain=False):
    """numpy [B, S, H, d] -> [o, lse, dq, dk, dv] numpy, every operand inside a NaN-filled allocation (odd: six different row strides, none a
    multiple of 4, and odd offsets); plain: seld_attn_fwd / _bwd instead.  Checks that nothing outside the windows is written."""
    HD, R = H * d, B * S
    band = 64 * HD + 1
    lds, fronts = _odd_strides(HD) if odd else ([HD] * 6, [band] * 6)
    span = max(lds)
    wq, wk, wv = (_Window(R, HD, ld, span, f, band, a) for ld, f, a in zip(lds[:3], fronts[:3], (q, k, v)))
    gq, gk, gv = (_Window(R, HD, ld, span, f, band) for ld, f in zip(lds[3:], fronts[3:]))
    wo, wl = _Window(R, HD, front=band, back=band), _Window(B * H, S, front=band, back=band)
    wd = _Window(1, lib.seld_attn_bwd_scratch(B, S, H, d), front=band, back=band)
    wg = _Window(R, HD, front=band, back=band, data=do)
    draws = () if plain else (rate, seed, layer, step)
    fwd, bwd = (lib.seld_attn_fwd, lib.seld_attn_bwd) if plain else (lib.seld_attn_drop_fwd, lib.seld_attn_drop_bwd)
    assert fwd(wq.ptr(), wk.ptr(), wv.ptr(), lds[0], lds[1], lds[2], wo.ptr(), wl.ptr(), B, S, H, d, scale, *draws, _stream()) == 0
    inputs = {"Q": wq, "K": wk, "V": wv, "dO": wg, "O": wo, "lse": wl}
    torch.cuda.synchronize()
    for w in inputs.values():
        w.snapshot()
    assert bwd(wq.ptr(), wk.ptr(), wv.ptr(), lds[0], lds[1], lds[2], wo.ptr(), wg.ptr(), wl.ptr(), gq.ptr(), gk.ptr(), gv.ptr(), lds[3], lds[4],
               lds[5], wd.ptr(), B, S, H, d, scale, *draws, _stream()) == 0
    torch.cuda.synchronize()
    for name, w in inputs.items():
        w.assert_unchanged(name)
        w.assert_band(name)
    for name, w in (("dQ", gq), ("dK", gk), ("dV", gv), ("delta scratch", wd)):
        w.assert_band(name)
    return [wo.numpy(), wl.numpy().reshape(B, H, S), gq.numpy(), gk.numpy(), gv.numpy()]


def _qkv(B, S, H, d, seed):
    rng = np.random.default_rng(seed)
    return [T.f32(rng.standard_normal((B, S, H, d))) for _ in range(4)]


NAMES = ("O", "lse", "dQ", "dK", "dV")
# (B, S, H, d): a single key; edge tiles; exactly one tile; one row past a tile; two tiles and an edge with S % 4 = 2
DROP_CASES = [(2, 1, 2, 8), (2, 31, 1, 24), (2, 33, 3, 8), (1, 64, 2, 64), (2, 65, 2, 16), (2, 130, 3, 48)]


@pytest.mark.parametrize("rate", [0.1, 0.5])
@pytest.mark.parametrize("B,S,H,d", DROP_CASES)
def test_attention_with_dropped_probabilities(seld_lib, B, S, H, d, rate):
    q, k, v, do = _qkv(B, S, H, d, 100 * S + d)
    scale, layer, step = 1.0 / math.sqrt(d), 4096 + 32 + 2, 7
    ref = DO.attention_reference(q, k, v, do, scale, rate, SEED, layer, step)
    got = _attn_drop(seld_lib, q, k, v, do, B, S, H, d, scale, rate, layer, step)
    biggest = max(np.abs(r).max() for r in ref[2:])
    for name, g, r in zip(NAMES, got, ref):
        if name in ("dQ", "dK"):
            _check_or_zero(f"drop {rate} {name}", g, r, biggest)      # S = 1: P = 1 and dS = M (dO . V) - delta = 0 exactly
        else:
            check(f"drop {rate} {name}", g, r)
    # strides move addresses only; a second run gives the same bits
    for a, b in zip(got, _attn_drop(seld_lib, q, k, v, do, B, S, H, d, scale, rate, layer, step, odd=True)):
        assert np.array_equal(a, b)
    # lse is the undropped softmax's, bit for bit
    plain = _attn_drop(seld_lib, q, k, v, do, B, S, H, d, scale, rate, layer, step, plain=True)
    assert np.array_equal(got[1], plain[1])


@pytest.mark.parametrize("B,S,H,d", DROP_CASES)
def test_attention_rate_zero_is_the_undropped_call_bit_for_bit(seld_lib, B, S, H, d):
    q, k, v, do = _qkv(B, S, H, d, 7 * S + d)
    scale = 1.0 / math.sqrt(d)
    for odd in (False, True):
        a = _attn_drop(seld_lib, q, k, v, do, B, S, H, d, scale, 0.0, 4096, 3, odd=odd)
        b = _attn_drop(seld_lib, q, k, v, do, B, S, H, d, scale, 0.0, 0, 0, odd=odd, plain=True)
        for name, x, y in zip(NAMES, a, b):
            assert np.array_equal(x, y), name


def test_attention_draws_follow_layer_and_step(seld_lib):
    B, S, H, d, rate = 2, 33, 3, 8, 0.1
    q, k, v, do = _qkv(B, S, H, d, 5)
    scale = 1.0 / math.sqrt(d)
    base = _attn_drop(seld_lib, q, k, v, do, B, S, H, d, scale, rate, 4098, 7)
    again = _attn_drop(seld_lib, q, k, v, do, B, S, H, d, scale, rate, 4098, 7)
    plain = _attn_drop(seld_lib, q, k, v, do, B, S, H, d, scale, rate, 0, 0, plain=True)
    for a, b in zip(base, again):
        assert np.array_equal(a, b)
    for layer, step, seed in ((4099, 7, SEED), (4098, 8, SEED), (4098, 7, SEED ^ 1), (4098, 7, SEED ^ (1 << 40))):
        other = _attn_drop(seld_lib, q, k, v, do, B, S, H, d, scale, rate, layer, step, seed=seed)
        assert not np.array_equal(other[0], base[0]) and not np.array_equal(other[4], base[4])
        assert np.array_equal(other[1], plain[1])      # lse never sees the mask
        check("another stream against its own oracle", other[0], DO.attention_reference(q, k, v, do, scale, rate, seed, layer, step)[0])
    assert not np.array_equal(base[0], plain[0])


# ---------------------------------------------------------------- the blocks through the factories
def _tf_cfg(rate):
    return {"depth": 1, "n_head": 2, "key_dim": 64, "ff_multiplier": 2, "kernel_size": 4, "dropout_rate": rate}


BLOCK_CASES = {
    "transformer": ("transformer", 2, 33, 40, 1, _tf_cfg),
    "transformer stage of 2": ("transformer", 2, 33, 40, 2, lambda r: dict(_tf_cfg(r), depth=2, key_dim=16, activation="swish")),
    "conformer": ("conformer", 2, 33, 50, 1, lambda r: dict(CF._cfg(5, 8, 8, 4, use_bias=False), dropout_rate=r)),
    "conformer stage of 2": ("conformer", 2, 33, 48, 2, lambda r: dict(CF._cfg(4, 16, 5, 2, depth=2, ffn_factor=1.0, activation="relu"), dropout_rate=r)),
    "attention lnf": ("attention", 2, 33, 32, 1, lambda r: dict(A._cfg(abs_pos_encoding=True, layer_norm_in_front=True, use_glu=True), dropout_rate=r)),
    "attention": ("attention", 2, 33, 32, 1, lambda r: dict(A._cfg(abs_pos_encoding=True, use_bias=True, kernel_size=4), dropout_rate=r)),
    "attention no tail": ("attention", 2, 33, 32, 1, lambda r: dict(A._cfg(abs_pos_encoding=True, kernel_size=0, use_glu=True, ff_factor0=0), dropout_rate=r)),
}


def _build(kind, cfg, B, S, D, depth, w, st):
    from seld_amd import modules
    name = {"transformer": "transformer_encoder", "conformer": "conformer_encoder", "attention": "attention"}[kind]
    stage = getattr(modules, name + ("_stage" if depth > 1 else "_block"))(cfg, dropout=True)((B, S, D))
    rt = stage.rt
    rt.finalize()
    rt.params[:rt.n_params].copy_(torch.as_tensor(w))
    if rt.n_state:
        rt.state[:rt.n_state].copy_(torch.as_tensor(st))
    return stage, rt


@pytest.mark.parametrize("case", list(BLOCK_CASES))
def test_block_training_forward_and_backward_with_dropout(case):
    kind, B, S, D, depth, mk = BLOCK_CASES[case]
    cfg, cfg0, step = mk(0.1), mk(0), 3
    ref = DO.stage_reference(kind, B, S, D, depth, cfg, seed=S + D, step=step)
    tr, nt = ref["specs"]
    stage, rt = _build(kind, cfg, B, S, D, depth, ref["w"], ref["st"])
    assert [(n, s) for n, _, s in rt.variables] == tr and [(n, s) for n, _, s in rt.state_variables] == nt
    assert rt.dropout_seed == SEED and rt.dropout_step == 0
    xd, dyd = dev(ref["x"].reshape(B * S, D)), dev(ref["dy"].reshape(B * S, D))
    # inference draws nothing: the bits of the same stage built with dropout_rate 0
    plain, _ = _build(kind, cfg0, B, S, D, depth, ref["w"], ref["st"])
    assert torch.equal(stage.forward(xd, B, False), plain.forward(xd, B, False)) and rt.dropout_step == 0
    rt.dropout_step = step
    out = stage.forward(xd, B, True).cpu().numpy().copy()
    assert (rt.dropout_cur, rt.dropout_step) == (step, step + 1)
    dx = stage.backward(dyd, B).cpu().numpy().copy()
    grads = rt.grads[:rt.n_params].cpu().numpy().copy()
    check(f"{case} forward", out, ref["out"].reshape(B * S, D))
    check(f"{case} input gradient", dx, ref["dx"].reshape(B * S, D))
    off, biggest = 0, float(np.abs(ref["grad"]).max())
    for n, s in tr:
        kk = int(np.prod(s))
        _check_or_zero(f"{case} grad {n}", grads[off:off + kk], ref["grad"][off:off + kk], biggest)
        off += kk
    # the next training forward draws new masks; the step set back gives the first one's bits again (BatchNormalization's batch statistics
    # do not depend on the moving ones)
    out2 = stage.forward(xd, B, True).cpu().numpy().copy()
    assert rt.dropout_cur == step + 1 and not np.array_equal(out2, out)
    rt.dropout_step = step
    assert np.array_equal(stage.forward(xd, B, True).cpu().numpy(), out)
    # it differs from the undropped training forward, and the caller's gradient was not written
    assert not np.array_equal(plain.forward(xd, B, True).cpu().numpy(), out)
    assert torch.equal(dyd, dev(ref["dy"].reshape(B * S, D)))


# ---------------------------------------------------------------- the model
def test_train_step_with_a_transformer_encoder_stage_and_dropout(seldnet_config):
    """models.seldnet with FIRST = mother_stage and SECOND = transformer_encoder_stage of depth 2 at dropout_rate 0.1: one train step at an
    explicitly set dropout_step against the oracle's — outputs, both losses, every gradient"""
    from oracle import seldnet_oracle as O
    from seld_amd import losses, models, train
    from test_modules_gpu import STAGE_FIRST
    cfg = copy.deepcopy(seldnet_config)
    cfg["FIRST"], cfg["FIRST_ARGS"] = "mother_stage", copy.deepcopy(STAGE_FIRST)
    cfg["SECOND"] = "transformer_encoder_stage"
    cfg["SECOND_ARGS"] = {"depth": 2, "n_head": 4, "key_dim": 24, "ff_multiplier": 2, "kernel_size": 1, "dropout_rate": 0.1}
    B, T_, step = 2, 50, 5
    in_shape = (B, T_, 64, 7)
    tr, nt = T.variable_specs(cfg, in_shape)
    w, st = T.random_weights(cfg, in_shape, seed=11)
    x, ys, yd = O.synthetic_batch(B, T_, seed=23)
    model = models.seldnet(in_shape, cfg)
    assert type(model).__name__ == "ComposedSeldNet" and [(n, s) for n, _, s in model.variables] == tr
    assert model.dropout_seed == SEED and model.dropout_step == 0
    model.set_weights(w, st)
    # inference: no draws, the step does not move; it is the dropout_rate 0 model's output bit for bit
    cfg0 = copy.deepcopy(cfg)
    cfg0["SECOND_ARGS"]["dropout_rate"] = 0
    model0 = models.seldnet(in_shape, cfg0)
    model0.set_weights(w, st)
    y_e, y_0 = model(x, training=False), model0(x, training=False)
    assert torch.equal(y_e[0], y_0[0]) and torch.equal(y_e[1], y_0[1]) and model.dropout_step == 0
    model.dropout_step = step
    ref = DO.transformer_model_train_step(cfg, in_shape, w, st, x, ys, yd, dropout_step=step)
    y_p, sl, dl = train.trainstep(model, x, (ys, yd), losses.BinaryCrossentropy(), losses.get_doa_loss("MSE"), (1.0, 1000.0), train.Adam(1e-3))
    assert model.dropout_step == step + 1
    check("dropout model trainstep sed", y_p[0].cpu().numpy(), ref["sed"])
    check("dropout model trainstep doa", y_p[1].cpu().numpy(), ref["doa"])
    check("dropout model sloss", sl.cpu().numpy(), ref["sloss"])
    check("dropout model dloss", dl.cpu().numpy(), ref["dloss"])
    g = model.get_grads()
    for n, off, sh in model.variables:
        k = int(np.prod(sh))
        r = ref["grad"][off:off + k]
        if np.abs(r).max() < 1e-9 * np.abs(ref["grad"]).max():      # conv biases in front of training-mode BatchNormalization; the key biases
            assert np.abs(g[off:off + k]).max() <= 1e-3 * np.abs(ref["grad"]).max(), n
            continue
        check(f"dropout model grad {n}", g[off:off + k], r)
    # the masks mattered: the dropout_rate 0 model's train step gives another output
    y_n, _, _ = train.trainstep(model0, x, (ys, yd), losses.BinaryCrossentropy(), losses.get_doa_loss("MSE"), (1.0, 1000.0), train.Adam(1e-3))
    assert float((y_n[0] - y_p[0]).abs().max()) > 1e-3 * float(np.abs(ref["sed"]).max())
