"""Every instantiation of the two kernel templates of seld_amd/csrc/gru.hip, one entry point at a time, against the fp64 restatement
tests/rnn_oracle.py at the staging-chunk edges of both kernels (16 forward steps, 8 backward) and under recurrent dropout:

  form    forward                                        backward
  k       seld_k_gru_fwd        <SAVE, PRIO> | <-, PRIO>   seld_k_gru_bwd        <PRIO, -, 0>   the 'mul' merge: dh = dout * h_other
  rnn2    seld_rnn_gru_fwd      the same two               seld_rnn_gru_bwd      <PRIO, -, 1>   the directions' output gradients as given
  rnn1    seld_rnn_gru_fwd      <SAVE | -, PRIO, -, UNI>   seld_rnn_gru_bwd      <PRIO, -, 2>   one direction (gx_b = NULL)
  drop    seld_k_gru_drop_fwd   <SAVE, -, DROP>            seld_k_gru_drop_bwd   <-, DROP, 0>   masked state, hm stored / read

The bar is helpers.check's 1e-4 (max|d| / max|ref|), applied by R.gru_compare per direction and per gate block: the z | r | h thirds of dgx and dgh
and the four planes z, r, hh, gh of the saved gates, which no other test compares with anything.  tests/test_rnn_cpu.py holds that a plain fp32
evaluation of every case here stays within 5e-5 at the same granularity, and that R.gru_compare reports three kinds of wrong kernel.

Every output sits in a NaN-filled allocation with a 512-float guard band in front and behind; inputs, bands included, must keep their bits."""
import functools

import numpy as np
import pytest
import torch

import rnn_oracle as R
from helpers import REL_TOL
from test_attention_gpu import _stream
from test_rnn_gpu import INVALID, UNSUPPORTED, _pad, _pair, _win

pytestmark = pytest.mark.gpu

PLAIN = ("k", "rnn2", "rnn1")


def _nd(form):
    return 1 if form == "rnn1" else 2


def _all_nan(w):
    return bool(torch.isnan(w.buf).all())


def _pad_rows(a, rows):
    a = np.asarray(a)
    return np.concatenate([a, np.zeros((rows - a.shape[0],) + a.shape[1:], a.dtype)]) if rows > a.shape[0] else a


def _forward(lib, form, ins, B, S, save=True, masks=None, Ba=None):
    """one forward entry -> {h, saved (when saving), hm (drop), out (k): [per direction] numpy}; Ba: the batch the buffers are sized for"""
    nd, Ba = _nd(form), Ba or B
    R_, Ra = B * S, Ba * S
    gx = [_win(Ra, 384, _pad(ins["gx"][d], B, Ba)) for d in range(nd)]
    U = [_win(128, 384, ins["U"][d]) for d in range(nd)]
    br = [_win(1, 384, ins["brec"][d]) for d in range(nd)]
    h, sv = [_win(Ra, 128) for _ in range(nd)], [_win(Ra, 512) for _ in range(nd)]
    inputs, outputs = gx + U + br, h + sv
    svp = _pair(sv, nd) if save else (None, None)
    if form == "drop":
        rm = [_win(Ba, 128, _pad_rows(masks[d], Ba)) for d in range(nd)]
        hm = [_win(Ra, 128) for _ in range(nd)]
        inputs, outputs = inputs + rm, outputs + hm
    if form == "k":
        out = _win(Ra, 128)
        outputs = outputs + [out]
    for w in inputs:
        w.snapshot()
    if form == "k":
        rc = lib.seld_k_gru_fwd(*_pair(gx, nd), *_pair(U, nd), *_pair(br, nd), *_pair(h, nd), *svp, out.ptr(), B, S, 128)
    elif form == "drop":
        rc = lib.seld_k_gru_drop_fwd(*_pair(gx, nd), *_pair(U, nd), *_pair(br, nd), *_pair(rm, nd), *_pair(h, nd), *_pair(hm, nd), *svp, B, S, 128)
    else:
        rc = lib.seld_rnn_gru_fwd(*_pair(gx, nd), *_pair(U, nd), *_pair(br, nd), *_pair(h, nd), *svp, B, S, 128, _stream())
    assert rc == 0, f"{form} forward: {rc}"
    torch.cuda.synchronize()
    for w in inputs:
        w.assert_unchanged(f"{form} forward input")
    for w in outputs:
        w.assert_band(f"{form} forward output")
        assert bool(torch.isnan(w.view[R_:]).all()), "rows of a clip that does not run were written"
    if not save:
        assert all(_all_nan(w) for w in sv), "saved = NULL, and a saved buffer was written"
    res = {"h": [w.numpy()[:R_].reshape(B, S, 128) for w in h]}
    if save:
        res["saved"] = [w.numpy()[:R_].reshape(B, S, 128, 4) for w in sv]
    if form == "drop":
        res["hm"] = [w.numpy()[:R_].reshape(B, S, 128) for w in hm]
    if form == "k":
        res["out"] = [out.numpy()[:R_].reshape(B, S, 128)]
    return res


def _backward(lib, form, ins, B, S, fw, dh=None, masks=None, Ba=None):
    """one backward entry on the forward values fw = {h, saved, hm (drop)} -> {dgx, dgh: [per direction] numpy}.  The mul-merged forms (k, drop)
    take dout = ins['dh'][0]; the others the per-direction output gradients dh (default ins['dh'])"""
    nd, Ba = _nd(form), Ba or B
    R_, Ra = B * S, Ba * S
    up = lambda a, cols: _win(Ra, cols, _pad(np.asarray(a).reshape(B, S, cols), B, Ba))
    h = [up(fw["h"][d], 128) for d in range(nd)]
    sv = [up(fw["saved"][d], 512) for d in range(nd)]
    U = [_win(128, 384, ins["U"][d]) for d in range(nd)]
    dgx, dgh = [_win(Ra, 384) for _ in range(nd)], [_win(Ra, 384) for _ in range(nd)]
    inputs = h + sv + U
    if form in ("k", "drop"):
        dout = up(ins["dh"][0], 128)
        inputs = inputs + [dout]
    else:
        wdh = [up((ins["dh"] if dh is None else dh)[d], 128) for d in range(nd)]
        inputs = inputs + wdh
    if form == "drop":
        rm = [_win(Ba, 128, _pad_rows(masks[d], Ba)) for d in range(nd)]
        hm = [up(fw["hm"][d], 128) for d in range(nd)]
        inputs = inputs + rm + hm
    for w in inputs:
        w.snapshot()
    if form == "k":
        rc = lib.seld_k_gru_bwd(dout.ptr(), *_pair(h, nd), *_pair(sv, nd), *_pair(U, nd), *_pair(dgx, nd), *_pair(dgh, nd), B, S, 128)
    elif form == "drop":
        rc = lib.seld_k_gru_drop_bwd(dout.ptr(), *_pair(h, nd), *_pair(hm, nd), *_pair(sv, nd), *_pair(U, nd), *_pair(rm, nd), *_pair(dgx, nd),
                                     *_pair(dgh, nd), B, S, 128)
    else:
        rc = lib.seld_rnn_gru_bwd(*_pair(wdh, nd), *_pair(h, nd), *_pair(sv, nd), *_pair(U, nd), *_pair(dgx, nd), *_pair(dgh, nd), B, S, 128, _stream())
    assert rc == 0, f"{form} backward: {rc}"
    torch.cuda.synchronize()
    for w in inputs:
        w.assert_unchanged(f"{form} backward input")
    for w in dgx + dgh:
        w.assert_band(f"{form} backward output")
        assert bool(torch.isnan(w.view[R_:]).all()), "rows of a clip that does not run were written"
    return {"dgx": [w.numpy()[:R_].reshape(B, S, 384) for w in dgx], "dgh": [w.numpy()[:R_].reshape(B, S, 384) for w in dgh]}


def _run(lib, form, ins, B, S, masks=None, Ba=None):
    fw = _forward(lib, form, ins, B, S, masks=masks, Ba=Ba)
    return {**fw, **_backward(lib, form, ins, B, S, fw, masks=masks, Ba=Ba)}


def _first(ref):
    """the forward direction alone of a gru_reference result"""
    return {k: v[:1] for k, v in ref.items()}


@functools.lru_cache(maxsize=None)
def _case(B, S, scale=1.0):
    """-> inputs, {form: fp64 reference}"""
    ins = R.recurrence_inputs("gru", B, S, scale)
    dh = R.gru_reference(ins)
    return ins, {"k": R.gru_reference(ins, mul=True), "rnn2": dh, "rnn1": _first(dh)}


@functools.lru_cache(maxsize=None)
def _drop_case(B, S):
    ins, masks = R.recurrence_inputs("gru", B, S), R.gru_drop_masks(B, R.GRU_DROP_RATE)
    return ins, masks, R.gru_reference(ins, rec_mask=masks, mul=True)


_DEVICE = {}


def _device(lib, B, S):
    """the three undropped forms' forward and backward outputs at (B, S), run once"""
    if (B, S) not in _DEVICE:
        ins, _ = _case(B, S)
        _DEVICE[(B, S)] = {form: _run(lib, form, ins, B, S) for form in PLAIN}
    return _DEVICE[(B, S)]


def _same_bits(tag, a, b, keys=None):
    for k in keys or a:
        assert len(a[k]) == len(b[k])
        for i, (x, y) in enumerate(zip(a[k], b[k])):
            assert np.isfinite(x).all() and np.array_equal(x, y), f"{tag}: {k}[{i}] differs"


# ---------------------------------------------------------------- every form at every edge
@pytest.mark.parametrize("B,S", R.GRU_EDGE_CASES)
def test_every_form_against_fp64_at_the_chunk_edges(seld_lib, B, S):
    """h, out, the saved gates, dgx and dgh of the mul-merged pair, the bidirectional pair with independent output gradients and the one-direction
    pair.  S: one below, at and one above one and two staging chunks of both kernels (the peeled last step, the double-buffered LDS images, h_prev
    across the chunk border, the step parity over odd chunks), and 53 = 3 forward / 6 backward chunks and a ragged tail"""
    _, refs = _case(B, S)
    got = _device(seld_lib, B, S)
    for form in PLAIN:
        R.gru_compare(f"gru {form} {(B, S)}", got[form], refs[form], REL_TOL)
    z, r, hh = (got["k"]["saved"][0][..., k] for k in range(3))
    assert (z > 0).all() and (z < 1).all() and (r > 0).all() and (r < 1).all() and (np.abs(hh) <= 1).all()


@pytest.mark.parametrize("B,S", R.GRU_EDGE_CASES)
def test_forms_agree_bit_for_bit(seld_lib, B, S):
    lib = seld_lib
    ins, _ = _case(B, S)
    got = _device(lib, B, S)
    # the three forward entries: the same h and saved gates
    _same_bits("seld_rnn_gru_fwd against seld_k_gru_fwd", got["k"], got["rnn2"], ("h", "saved"))
    _same_bits("one direction against seld_k_gru_fwd", _first(got["k"]), got["rnn1"], ("h", "saved"))
    # saved = NULL: the no-save instantiations (bidirectional through both entries, one-direction) give the same h and write no saved buffer
    for form in PLAIN:
        _same_bits(f"{form} without saving", got[form], _forward(lib, form, ins, B, S, save=False), ("h",))
    # the 'mul' merge formed outside in fp32, as the mul-merged kernel forms it
    dout, h = ins["dh"][0], got["k"]["h"]
    as_given = _backward(lib, "rnn2", ins, B, S, got["k"], dh=[dout * h[1], dout * h[0]])
    _same_bits("seld_rnn_gru_bwd on dout * h_other against seld_k_gru_bwd", got["k"], as_given, ("dgx", "dgh"))
    # a second run
    for form in PLAIN:
        _same_bits(f"{form}, a second run", got[form], _run(lib, form, ins, B, S))


# ---------------------------------------------------------------- the backward kernels alone
@pytest.mark.parametrize("S", R.GRU_BPTT_S)
def test_isolated_bptt_on_the_oracles_forward_values(seld_lib, S):
    """each backward form on the fp64 oracle's h, hm and saved gates rounded to fp32, not on what the device's forward left: a forward error (a wrong
    value or a wrong layout of the saved gates) cannot be mirrored by the backward"""
    B = 2
    ins, refs = _case(B, S)
    for form in PLAIN:
        ref, nd = refs[form], _nd(form)
        fw = {"h": [R.f32(ref["h"][d]) for d in range(nd)], "saved": [R.f32(R.gru_saved(ref, d)) for d in range(nd)]}
        R.gru_compare(f"bptt {form} {(B, S)}", _backward(seld_lib, form, ins, B, S, fw), ref, REL_TOL)
    B = R.GRU_DROP_BPTT_CASES[0][0]
    assert (B, S) in R.GRU_DROP_BPTT_CASES
    ins, masks, ref = _drop_case(B, S)
    fw = {"h": [R.f32(a) for a in ref["h"]], "hm": [R.f32(a) for a in ref["hm"]], "saved": [R.f32(R.gru_saved(ref, d)) for d in (0, 1)]}
    R.gru_compare(f"bptt drop {(B, S)}", _backward(seld_lib, "drop", ins, B, S, fw, masks=masks), ref, REL_TOL)


# ---------------------------------------------------------------- recurrent dropout
@pytest.mark.parametrize("B,S", R.GRU_DROP_CASES + R.GRU_DROP_AT_CHUNKS)
def test_dropout_forms_against_fp64(seld_lib, B, S):
    """seld_k_gru_drop_fwd / _bwd, rate 0.2: h (unmasked), hm (the masked state sequence), the saved gates, dgx, dgh"""
    ins, masks, ref = _drop_case(B, S)
    got = _run(seld_lib, "drop", ins, B, S, masks=masks)
    R.gru_compare(f"gru drop {(B, S)}", got, ref, REL_TOL)
    for d in (0, 1):
        m = masks[d][:, None, :]
        assert np.array_equal(got["hm"][d], got["h"][d] * m), f"hm[{d}] is not h * mask in fp32"
        dropped = np.broadcast_to(m == 0, got["hm"][d].shape)
        assert dropped.any() and (got["hm"][d][dropped] == 0).all()
    _same_bits("drop, a second run", got, _run(seld_lib, "drop", ins, B, S, masks=masks))


@pytest.mark.parametrize("B,S", R.GRU_EDGE_CASES)
def test_dropout_forms_with_all_ones_masks_equal_the_undropped_kernels(seld_lib, B, S):
    """a mask of ones multiplies the new state and the carry by 1: the bits of the undropped kernels, which differ in the issue priority alone; this
    also runs the dropout instantiations at every chunk edge"""
    ins, _ = _case(B, S)
    got = _run(seld_lib, "drop", ins, B, S, masks=np.ones((2, B, 128), np.float32))
    _same_bits("all-ones masks against the undropped kernels", _device(seld_lib, B, S)["k"], got, ("h", "saved", "dgx", "dgh"))
    _same_bits("hm against h", {"h": got["h"]}, {"h": got["hm"]})


def test_dropout_entries_refuse_and_write_nothing(seld_lib):
    """units != 128 -> UNSUPPORTED before any other check; a NULL pointer (a half-given mask set among them), B < 1, S < 1 -> INVALID; nothing runs"""
    lib, B, S = seld_lib, 2, 5
    g = [_win(B * S, 384) for _ in range(6)]       # gx_f gx_b dgx_f dgx_b dgh_f dgh_b
    U, br, rm = ([_win(r, c) for _ in (0, 1)] for r, c in ((128, 384), (1, 384), (B, 128)))
    h, hm, sv = ([_win(B * S, c) for _ in (0, 1)] for c in (128, 128, 512))
    dout = _win(B * S, 128)
    p = lambda ws: _pair(ws, 2)
    fwd = [*p(g[0:2]), *p(U), *p(br), *p(rm), *p(h), *p(hm), *p(sv)]
    bwd = [dout.ptr(), *p(h), *p(hm), *p(sv), *p(U), *p(rm), *p(g[2:4]), *p(g[4:6])]
    for fn, args in ((lib.seld_k_gru_drop_fwd, fwd), (lib.seld_k_gru_drop_bwd, bwd)):
        assert fn(*args, B, S, 64) == UNSUPPORTED
        assert fn(*[None] * len(args), 0, 0, 64) == UNSUPPORTED
        for i in range(len(args)):      # each pointer in turn: rm_f alone, rm_b alone, ...
            assert fn(*args[:i], None, *args[i + 1:], B, S, 128) == INVALID, f"{fn.__name__}: argument {i} is NULL"
        assert fn(*args, 0, S, 128) == INVALID and fn(*args, B, 0, 128) == INVALID and fn(*args, -1, S, 128) == INVALID
    torch.cuda.synchronize()
    for w in g + U + br + rm + h + hm + sv + [dout]:
        assert _all_nan(w), "a refused call wrote"


# ---------------------------------------------------------------- batch mapping
def test_every_clip_of_a_batch_equals_that_clip_alone(seld_lib):
    """B = 5 distinct clips at S = 17: the workgroup -> (clip, direction) mapping (blockIdx >> 1 | blockIdx & 1, and blockIdx in the one-direction
    instantiations) and every per-clip base offset, the masks' included"""
    B, S = R.GRU_BATCH_CASE
    ins, refs = _case(B, S)
    _, masks, dref = _drop_case(B, S)
    for form in PLAIN + ("drop",):
        m = masks if form == "drop" else None
        whole = _run(seld_lib, form, ins, B, S, masks=m)
        R.gru_compare(f"gru {form} {(B, S)}", whole, dref if form == "drop" else refs[form], REL_TOL)
        for b in range(B):
            one = {k: (v[:, b:b + 1] if k in ("gx", "dh") else v) for k, v in ins.items()}
            alone = _run(seld_lib, form, one, 1, S, masks=None if m is None else m[:, b:b + 1])
            _same_bits(f"{form}: clip {b} of {B} against the clip alone", {k: [a[b:b + 1] for a in v] for k, v in whole.items()}, alone)


# ---------------------------------------------------------------- robustness
def test_smaller_batch_on_buffers_sized_for_a_larger_one(seld_lib):
    """B = 2 on buffers sized for 3: the rows of the third clip stay NaN (asserted in _forward / _backward), the rest is what exact buffers give"""
    B, S, Ba = R.GRU_SMALLER_BATCH
    ins, refs = _case(B, S)
    for form in PLAIN:
        got = _run(seld_lib, form, ins, B, S, Ba=Ba)
        R.gru_compare(f"gru {form} b < B", got, refs[form], REL_TOL)
        _same_bits(f"{form}: b < B against exact buffers", _device(seld_lib, B, S)[form], got)
    masks = R.gru_drop_masks(B, R.GRU_DROP_RATE)
    _same_bits("drop: b < B against exact buffers", _run(seld_lib, "drop", ins, B, S, masks=masks), _run(seld_lib, "drop", ins, B, S, masks=masks, Ba=Ba))


def test_saturated_gates_stay_finite(seld_lib):
    B, S, scale = R.GRU_SATURATED
    ins, refs = _case(B, S, scale)
    assert np.abs(ins["gx"]).max() > 30
    for form in PLAIN:
        got = _run(seld_lib, form, ins, B, S)
        assert all(np.isfinite(a).all() for v in got.values() for a in v), form
        R.gru_compare(f"gru {form} x{scale}", got, refs[form], REL_TOL)
