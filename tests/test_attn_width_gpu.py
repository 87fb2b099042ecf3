"""The any-width attention on the device: seld_attnw_* (seld_amd/csrc/attention.hip) against transformer_oracle.attention in fp64 at the
project's bar (helpers.check: max|d| / max|ref| <= 1e-4; test_attention_gpu's rule for gradients that are zero by mathematics) over the head
widths and lengths of tests/attn_width_cases.py, contiguous and as column slices of one fused buffer with NaN guard columns; the design's
invariant — the values of seld_attn_* at the padded width on zero-padded operands, bit for bit, with and without dropped probabilities;
then the blocks and the model that route to it (modules' any_key_dim, ConvTemporalNet search=True) and the search's main with
--attention_stages on a tiny data set."""
import json
import math
import os

import numpy as np
import pytest
import torch

import attn_width_cases as A
import conformer_oracle as K
import conv_temporal_oracle as CT
import transformer_oracle as T
from helpers import check, dev, ptr
from test_attention_gpu import _check_or_zero, _stream

pytestmark = pytest.mark.gpu

B, H = A.B, A.H
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
nan = lambda *shape: torch.full(shape, float("nan"), device="cuda")


def _run(lib, entry, ops, S, d, fused=False, save=True, drop=None, scale=None):
    """ops: q, k, v, do as numpy [B, S, H, d] -> [o, lse, dq, dk, dv] numpy (save=False: o alone).  entry: 'seld_attn' or 'seld_attnw';
    drop: (rate, seed, layer, step) -> the *_drop_* entries.  fused: Q, K, V are column slices of one NaN-filled [B*S, 3 H d + GUARD] buffer and
    dQ, dK, dV of another; the guard columns behind them hold their NaNs after the calls"""
    q, k, v, do = ops
    HD, R = H * d, B * S
    scale = 1.0 / math.sqrt(d) if scale is None else scale
    if fused:
        ld = 3 * HD + A.GUARD
        buf, gbuf = nan(R, ld), nan(R, ld)
        views = [buf[:, i * HD:(i + 1) * HD] for i in range(3)]
        gviews = [gbuf[:, i * HD:(i + 1) * HD] for i in range(3)]
        for t, a in zip(views, (q, k, v)):
            t.copy_(dev(a.reshape(R, HD)))
    else:
        ld = HD
        views = [dev(a.reshape(R, HD)) for a in (q, k, v)]
        gviews = [nan(R, HD) for _ in range(3)]
    o, lse = nan(R, HD), nan(B, H, S) if save else None
    tail = list(drop or ()) + [_stream()]
    fwd = getattr(lib, entry + ("_drop_fwd" if drop else "_fwd"))
    assert fwd(ptr(views[0]), ptr(views[1]), ptr(views[2]), ld, ld, ld, ptr(o), ptr(lse), B, S, H, d, scale, *tail) == 0
    if not save:
        torch.cuda.synchronize()
        return o.cpu().numpy()
    n = getattr(lib, entry + "_bwd_scratch")(B, S, H, d)
    assert n == B * H * S
    scratch, god = nan(n), dev(do.reshape(R, HD))
    bwd = getattr(lib, entry + ("_drop_bwd" if drop else "_bwd"))
    assert bwd(ptr(views[0]), ptr(views[1]), ptr(views[2]), ld, ld, ld, ptr(o), ptr(god), ptr(lse), ptr(gviews[0]), ptr(gviews[1]),
               ptr(gviews[2]), ld, ld, ld, ptr(scratch), B, S, H, d, scale, *tail) == 0
    torch.cuda.synchronize()
    if fused:      # the guard columns were not touched, the operands hold what they held
        assert bool(torch.isnan(gbuf[:, 3 * HD:]).all()) and bool(torch.isnan(buf[:, 3 * HD:]).all())
        for t, a in zip(views, (q, k, v)):
            assert torch.equal(t, dev(a.reshape(R, HD)))
    assert bool(torch.isfinite(scratch).all())
    return [o.cpu().numpy(), lse.cpu().numpy()] + [g.contiguous().cpu().numpy() for g in gviews]


def _same_bits(tag, a, b):
    for name, x, y in zip(A.NAMES, a, b):
        assert np.array_equal(bits(x), bits(y)), f"{tag}: {name} differs"


@pytest.mark.parametrize("d,S", A.PARITY_CASES)
def test_parity_contiguous_and_fused(seld_lib, d, S):
    ops, ref = A.inputs(S, d), A.reference(S, d)
    runs = {fused: _run(seld_lib, "seld_attnw", ops, S, d, fused) for fused in (False, True)}
    biggest = max(np.abs(r).max() for r in ref[2:])
    for fused, got in runs.items():
        for name, g, r in zip(A.NAMES, got, ref):
            tag = f"attnw d={d} S={S} {'fused' if fused else 'contiguous'} {name}"
            assert np.isfinite(g).all(), tag
            if name in ("dQ", "dK"):
                _check_or_zero(tag, g, r, biggest)      # S = 1: dQ = dK = 0 exactly
            else:
                check(tag, g, r)
    _same_bits(f"d={d} S={S} fused against contiguous", runs[False], runs[True])
    _same_bits(f"d={d} S={S} second run", runs[False], _run(seld_lib, "seld_attnw", ops, S, d))
    for fused in (False, True):
        o = _run(seld_lib, "seld_attnw", ops, S, d, fused, save=False)
        assert np.array_equal(bits(o), bits(runs[False][0])), f"d={d} S={S}: O differs without lse"


def _padded_case(lib, d, S, drop):
    ops = A.inputs(S, d)
    dp = A.padded(d)
    scale = 1.0 / math.sqrt(d)
    got = _run(lib, "seld_attnw", ops, S, d, drop=drop, scale=scale)
    wide = _run(lib, "seld_attn", tuple(A.zero_padded(a, d) for a in ops), S, dp, drop=drop, scale=scale)
    tag = f"d={d} (dp={dp}) S={S}" + (" dropped" if drop else "")
    for name, g, w in zip(A.NAMES, got, wide):
        w = w if name == "lse" else A.head_columns(w, S, dp, d)
        assert g.shape == w.shape and np.array_equal(g, w), f"{tag}: {name} is not the padded call's"      # as floats: -0 == +0
    return got, wide


@pytest.mark.parametrize("S", A.PADDED_S)
@pytest.mark.parametrize("d", A.PADDED_D)
def test_padded_equivalence(seld_lib, d, S):
    """seld_attnw_* at d gives what seld_attn_* at 8 ceil(d / 8) gives on zero-padded operands with the same scale, and the padded call's
    gradients are zero in the columns the ragged call does not have"""
    _, wide = _padded_case(seld_lib, d, S, None)
    dp = A.padded(d)
    for name, w in zip(A.NAMES[2:], wide[2:]):
        assert not w.reshape(B * S, H, dp)[:, :, d:].any(), name


@pytest.mark.parametrize("S", A.PADDED_S)
@pytest.mark.parametrize("d", A.PADDED_D)
def test_padded_equivalence_with_dropped_probabilities(seld_lib, d, S):
    """the mask does not see d: seld_attnw_drop_* at d against seld_attn_drop_* at the padded width, same rate, seed, layer and step; and
    the dropped result differs from the undropped one while lse does not"""
    got, _ = _padded_case(seld_lib, d, S, A.DROP)
    plain = _run(seld_lib, "seld_attnw", A.inputs(S, d), S, d)
    assert np.array_equal(bits(got[1]), bits(plain[1])), "lse is the full softmax's"
    assert not np.array_equal(got[0], plain[0]) and not np.array_equal(got[4], plain[4])


@pytest.mark.parametrize("d", A.MULTIPLES)
def test_multiples_of_8_give_the_bits_of_the_narrow_entries(seld_lib, d):
    S = 65
    ops = A.inputs(S, d)
    for drop in (None, A.DROP):
        for fused in (False, True):
            _same_bits(f"d={d} drop={drop} fused={fused}", _run(seld_lib, "seld_attnw", ops, S, d, fused, drop=drop),
                       _run(seld_lib, "seld_attn", ops, S, d, fused, drop=drop))


@pytest.mark.parametrize("d", [3, 12, 33])
def test_rate_0_gives_the_bits_of_the_undropped_entries(seld_lib, d):
    S = 65
    ops = A.inputs(S, d)
    _same_bits(f"d={d} rate 0", _run(seld_lib, "seld_attnw", ops, S, d, drop=(0.0,) + A.DROP[1:]), _run(seld_lib, "seld_attnw", ops, S, d))
    assert np.array_equal(bits(_run(seld_lib, "seld_attnw", ops, S, d, save=False, drop=(0.0,) + A.DROP[1:])),
                          bits(_run(seld_lib, "seld_attnw", ops, S, d, save=False)))


# ---------------------------------------------------------------- blocks through seld_amd.modules
def _search_rt():
    from seld_amd import modules
    rt = modules._Rt(torch.device("cuda", torch.cuda.current_device()))
    rt.any_key_dim = True
    return rt


def _check_grads(tag, grads, ref_grad, specs):
    off, biggest = 0, float(np.abs(ref_grad).max())
    for n, s in specs:
        kk = int(np.prod(s))
        _check_or_zero(f"{tag} grad {n}", grads[off:off + kk], ref_grad[off:off + kk], biggest)
        off += kk


def test_transformer_encoder_block_at_key_dim_3():
    from oracle import seldnet_oracle as O
    from seld_amd import modules
    Bm, S, D, cfg = A.TRANSFORMER_BLOCK
    with pytest.raises(ValueError, match="multiple of 8"):
        modules._build_second("transformer_encoder_block", modules._Rt(torch.device("cuda", torch.cuda.current_device())), cfg, S, D, Bm, prefix="tf")
    stage = modules._build_second("transformer_encoder_block", _search_rt(), cfg, S, D, Bm, prefix="tf")
    assert stage.blocks[0].mha.wide and stage.blocks[0].mha.dk == 3
    rt = stage.blocks[0].rt
    rt.finalize()
    specs = T.stage_specs(D, cfg, 1)
    assert [(n, s) for n, _, s in rt.variables] == specs and rt.n_state == 0
    w = T.random_block_weights(specs, 3)
    rng = np.random.default_rng(3)
    x, dy = T.f32(rng.standard_normal((Bm, S, D))), T.f32(rng.standard_normal((Bm, S, D)))
    rt.params[:rt.n_params].copy_(torch.as_tensor(w))
    xd = dev(x.reshape(Bm * S, D))
    out_eval = stage.forward(xd, Bm, False).cpu().numpy().copy()
    out = stage.forward(xd, Bm, True).cpu().numpy().copy()
    dx = stage.backward(dev(dy.reshape(Bm * S, D)), Bm).cpu().numpy().copy()
    grads = rt.grads[:rt.n_params].cpu().numpy().copy()
    fw = torch.tensor(w, dtype=torch.float64, requires_grad=True)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    yt = T.stage_forward(xt, O.unflatten(fw, specs), cfg, 1)
    gw, gx = torch.autograd.grad((yt * torch.tensor(dy, dtype=torch.float64)).sum(), (fw, xt))
    tag = "transformer_encoder_block H2 dk3"
    check(f"{tag} forward", out, yt.detach().numpy().reshape(Bm * S, D))
    assert np.array_equal(out, out_eval)      # no dropout, no batch statistics
    check(f"{tag} input gradient", dx, gx.numpy().reshape(Bm * S, D))
    _check_grads(tag, grads, gw.numpy(), specs)


def test_conformer_encoder_block_at_key_dim_6():
    from seld_amd import modules
    Bm, S, D, cfg = A.CONFORMER_BLOCK
    with pytest.raises(ValueError, match="multiple of 8"):
        modules._build_second("conformer_encoder_block", modules._Rt(torch.device("cuda", torch.cuda.current_device())), cfg, S, D, Bm, prefix="cf")
    ref = K.stage_reference(Bm, S, D, 1, cfg, seed=3)
    tr, nt = ref["specs"]
    stage = modules._build_second("conformer_encoder_block", _search_rt(), cfg, S, D, Bm, prefix="cf")
    assert stage.blocks[0].mha.wide and stage.blocks[0].mha.dk == 6
    rt = stage.blocks[0].rt
    rt.finalize()
    assert [(n, s) for n, _, s in rt.variables] == tr and [(n, s) for n, _, s in rt.state_variables] == nt
    rt.params[:rt.n_params].copy_(torch.as_tensor(ref["w"]))
    rt.state[:rt.n_state].copy_(torch.as_tensor(ref["st"]))
    xd = dev(ref["x"].reshape(Bm * S, D))
    out = stage.forward(xd, Bm, True).cpu().numpy().copy()
    state = rt.state[:rt.n_state].cpu().numpy().copy()
    out_eval = stage.forward(xd, Bm, False).cpu().numpy().copy()
    rt.state[:rt.n_state].copy_(torch.as_tensor(ref["st"]))
    stage.forward(xd, Bm, True)
    dx = stage.backward(dev(ref["dy"].reshape(Bm * S, D)), Bm).cpu().numpy().copy()
    grads = rt.grads[:rt.n_params].cpu().numpy().copy()
    tag = "conformer_encoder_block H3 dk6"
    check(f"{tag} forward (training)", out, ref["out_train"].reshape(Bm * S, D))
    check(f"{tag} moving statistics", state, ref["new_state"])
    check(f"{tag} forward (inference)", out_eval, ref["out_eval"].reshape(Bm * S, D))
    check(f"{tag} input gradient", dx, ref["dx"].reshape(Bm * S, D))
    _check_grads(tag, grads, ref["grad"], tr)


# ---------------------------------------------------------------- the model
def test_model_against_the_oracle():
    """inference and one train step (outputs, both losses, the flat gradient, every variable's gradient, the BatchNormalization state)"""
    from seld_amd import losses, models, train
    w, st, x, ys, yd, ref = A.model_reference()
    tr, nt = CT.variable_specs(A.CONFIG, A.INPUT)
    model = models.conv_temporal(A.INPUT, A.CONFIG, search=True)
    assert [(n, s) for n, _, s in model.variables] == tr and [(n, s) for n, _, s in model.state_variables] == nt
    assert model.body[0].blocks[0].mha.wide and model.heads[0].body.blocks[0].mha.wide
    model.set_weights(w, st)
    tag = "conv_temporal key_dim 6 / 12"
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
    check(f"{tag} BN state", model.get_weights()[1], ref["new_state"])
    model.close()


def _two_steps(cfg):
    from seld_amd import losses, models, train
    w, st = CT.random_weights(cfg, A.INPUT, seed=11)
    x, ys, yd = CT.synthetic_batch(cfg, A.INPUT, seed=23)
    model = models.conv_temporal(A.INPUT, cfg, search=True)
    model.set_weights(w, st)
    opt = train.Adam(1e-3)
    outs = []
    for _ in range(2):
        y_p, sl, dl = train.trainstep(model, x, (ys, yd), losses.BinaryCrossentropy(), losses.MSE, (1.0, 1000.0), opt)
        outs += [y_p[0].cpu().numpy(), y_p[1].cpu().numpy(), sl.cpu().numpy(), dl.cpu().numpy(), model.get_grads()]
    outs += list(model.get_weights())
    model.close()
    return outs


def test_model_with_dropout_is_seeded():
    """dropout_rate 0.1 in both attention stages (the probabilities' masks inside seld_attnw_drop_*): two models from one seed agree bit for
    bit after two steps, and differ from rate 0"""
    a, b, zero = _two_steps(A.with_dropout(0.1)), _two_steps(A.with_dropout(0.1)), _two_steps(A.with_dropout(0.0))
    for i, (p, q) in enumerate(zip(a, b)):
        assert np.isfinite(p).all() and np.array_equal(bits(p), bits(q)), f"quantity {i} differs between two runs"
    assert not np.array_equal(a[0], zero[0]) and not np.array_equal(a[4], zero[4]) and not np.array_equal(a[-2], zero[-2])


# ---------------------------------------------------------------- the search's main
def test_nas_seldnet_main_with_attention_stages(tmp_path, monkeypatch):
    from seld_amd import nas_seldnet as N
    nc, F, Cc, win, fpl = 3, 8, 7, 4, 5      # input [20, 8, 7]: 4 labels of 5 frames
    rng = np.random.default_rng(5)
    for d in ("foa_dev_norm", "foa_dev_label"):
        os.makedirs(tmp_path / d)
    for fold in (1, 2, 6):
        L = 2 * win
        np.save(tmp_path / "foa_dev_norm" / f"fold{fold}_a.npy", T.f32(rng.standard_normal((L * fpl, F, Cc))))
        sed = (rng.random((L, nc)) < 0.3).astype(np.float32)
        doa = T.f32(rng.uniform(-1, 1, (L, 3 * nc))) * np.tile(sed, 3)
        np.save(tmp_path / "foa_dev_label" / f"fold{fold}_a.npy", np.concatenate([sed, doa], -1))
    monkeypatch.setattr(N, "search_space_2d", {"mother_stage": {
        "depth": [1], "filters0": [0], "filters1": [4, 6], "filters2": [0], "kernel_size0": [1], "kernel_size1": [1, 3], "kernel_size2": [1],
        "connect0": [[0], [1]], "connect1": [[0, 0], [1, 0]], "connect2": [[0, 0, 0], [1, 0, 1]], "strides": [(1, 2)]}})
    monkeypatch.setattr(N, "search_space_1d", {"bidirectional_GRU_stage": {"depth": [1], "units": [4, 12]}})
    monkeypatch.setattr(N, "search_space_1d_attention", {
        "transformer_encoder_stage": {"depth": [1], "n_head": [1, 2], "key_dim": [3, 8], "ff_multiplier": [0.5, 1], "kernel_size": [1, 3]},
        "conformer_encoder_stage": {"depth": [1], "key_dim": [3, 8], "n_head": [1, 2], "kernel_size": [4, 96], "multiplier": [1],
                                    "pos_encoding": [None, "basic", "rff"]}})
    name = str(tmp_path / "run")
    argv = ["--name", name, "--dataset_path", str(tmp_path), "--n_samples", "3", "--n_blocks", "2", "--min_flops", "0", "--max_flops", "0",
            "--batch_size", "2", "--n_repeat", "2", "--n_classes", str(nc), "--label_window_size", str(win), "--time_mask_size", "4",
            "--freq_mask_size", "3", "--attention_stages"]
    res = N.main(argv)
    with open(name + ".json") as f:
        assert json.load(f) == json.loads(json.dumps(res))
    assert sorted(k for k in res if k.isdigit()) == ["000", "001", "002"] and res["train_config"]["attention_stages"] is True
    keys = {"loss", "val_loss", "test_error_rate", "test_f1score", "test_der", "test_derf", "test_seld_score", "flops", "params", "time"}
    kinds, key_dims = [], set()
    for k in ("000", "001", "002"):
        perf, cfg = res[k]["perf"], res[k]["config"]
        assert set(perf) == keys, set(perf) ^ keys
        assert all(np.isfinite(np.asarray(v, np.float64)).all() for v in perf.values()), perf
        for b in ("BLOCK0", "BLOCK1", "SED", "DOA"):
            kinds.append(cfg[b])
            a = cfg[f"{b}_ARGS"]
            if cfg[b] in N.search_space_1d_attention:
                key_dims.add(a["key_dim"])
            if cfg[b] == "conformer_encoder_stage":      # what has no kernel was rejected, not built as something else
                assert a["kernel_size"] == 4 and a["pos_encoding"] in (None, "basic")
    assert set(kinds) & set(N.search_space_1d_attention), "the seeded draws hold no attention stage"
    assert 3 in key_dims, "the seeded draws hold no key_dim 3: the run did not reach seld_attnw_*"
