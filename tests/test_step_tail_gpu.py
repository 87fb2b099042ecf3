"""loss_adam.hip kernel by kernel on the device against tests/step_tail_oracle.py (float64): the losses at workgroup edges, with the fused heads'
row strides and the deferred finalize; Adam at block edges and late steps; AGC on one variable of every rank; the heads' activation backward,
the seldnet_v1 coupling, the Conv1D time layout, the float4 dropout, the per-clip masks and the fill.  Every operand sits in a NaN-filled
allocation (test_attention_gpu._Window): outputs start as NaN, inputs must keep their bits, and no float outside a window may change.
tests/test_step_tail_cpu.py holds the float32 room under every bar used here and the kernel -> test table."""
import ctypes as C

import numpy as np
import pytest
import torch

import step_tail_oracle as T
from helpers import check, dev
from test_attention_gpu import NAN_BITS, _bits, _Window

pytestmark = pytest.mark.gpu

FRONT, BACK = 68, 36      # floats around every window; multiples of 4: the float4 kernels need 16-byte aligned operands


def _in(a, cols=None):
    a = np.ascontiguousarray(a, np.float32)
    cols = a.shape[-1] if cols is None else cols
    w = _Window(a.size // cols, cols, front=FRONT, back=BACK, data=a)
    w.snapshot()
    return w


def _out(rows, cols, ld=None):
    return _Window(rows, cols, ld=ld, front=FRONT, back=BACK)


def _same_bits(name, a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, name
    n = int((a.view(np.uint32) != b.view(np.uint32)).sum())
    assert n == 0, f"{name}: {n} of {a.size} floats differ in their bits"


def _all_nan_bits(t):
    return bool((_bits(t.contiguous()) == NAN_BITS).all())


def _cfg(mode, den=0.0):
    from seld_amd import _lib
    return _lib.LossCfg(T.LOSS_MODES[mode], T.LOSS_WEIGHT[0], T.LOSS_WEIGHT[1], 1.0, den)


class _Losses:
    """one set of device operands for seld_k_losses_strided / seld_k_losses_finalize"""

    def __init__(self, lib, sed, doa, ys, yd, mode, strided=False, grads=True, den=0.0):
        self.lib, self.mode, self.cfg = lib, mode, _cfg(mode, den)
        self.B, self.S, self.nc = sed.shape
        rows, nc = self.B * self.S, self.nc
        self.rows = rows
        self.ins = [_in(sed), _in(doa), _in(ys), _in(yd)]
        self.sl, self.dl = _out(1, 1), _out(1, 1 if mode == "MMSE" else rows)
        self.scr = _out(1, int(lib.seld_m_losses_scratch(rows)))
        self.strided, self.grads = strided, grads
        if strided:       # api.hip's layout with room behind: [rows][4 nc + 8], dsed_pre at column 0, ddoa_pre at column nc
            self.ld = 4 * nc + 8
            self.g = _out(rows, self.ld)
            self.ps, self.pd = self.g.ptr(), C.c_void_p(self.g.view.data_ptr() + 4 * nc)
        elif grads:
            self.ld = 0
            self.gs, self.gd = _out(rows, nc), _out(rows, 3 * nc)
            self.ps, self.pd = self.gs.ptr(), self.gd.ptr()
        else:
            self.ld, self.ps, self.pd = 0, None, None

    def run(self, defer=0):
        a = [w.ptr() for w in self.ins]
        rc = self.lib.seld_k_losses_strided(*a, C.byref(self.cfg), self.sl.ptr(), self.dl.ptr(), self.ps, self.ld, self.pd, self.ld, self.scr.ptr(),
                                            self.B, self.S, self.nc, defer)
        assert rc == 0
        torch.cuda.synchronize()
        return self

    def finalize(self):
        assert self.lib.seld_k_losses_finalize(C.byref(self.cfg), self.sl.ptr(), self.dl.ptr(), self.scr.ptr(), self.B, self.S, self.nc) == 0
        torch.cuda.synchronize()
        return self

    def results(self):
        name = f"losses {self.mode} {self.B, self.S, self.nc}"
        for w in self.ins:
            w.assert_unchanged(name)
        for w in (self.sl, self.dl, self.scr):
            w.assert_band(name)
        r = {"sloss": self.sl.numpy().reshape(-1), "dloss": self.dl.numpy().reshape(-1)}
        nc = self.nc
        if self.strided:
            self.g.assert_band(name)
            assert _all_nan_bits(self.g.view[:, 4 * nc:]), f"{name}: a column behind the two gradients was written"
            r["dsed_pre"], r["ddoa_pre"] = self.g.view[:, :nc].cpu().numpy(), self.g.view[:, nc:4 * nc].cpu().numpy()
        elif self.grads:
            self.gs.assert_band(name)
            self.gd.assert_band(name)
            r["dsed_pre"], r["ddoa_pre"] = self.gs.numpy(), self.gd.numpy()
        return r


def _check_losses(name, got, ref, keys=tuple(T.TOL)):
    return {k: check(f"{name} {k}", got[k].reshape(-1), ref[k].reshape(-1), tol=T.TOL[k]) for k in keys}


@pytest.mark.parametrize("mode", sorted(T.LOSS_MODES))
@pytest.mark.parametrize("B,S,nc", T.LOSS_SHAPES)
def test_losses_against_fp64(seld_lib, B, S, nc, mode):
    sed, doa, ys, yd = T.loss_inputs(B, S, nc)
    got = _Losses(seld_lib, sed, doa, ys, yd, mode).run().results()
    _check_losses(f"losses {mode} {B, S, nc}", got, T.losses_ref(sed, doa, ys, yd, mode))
    if mode == "MAE":       # d|e| at e = 0 is 0: exactly, 0 = 0 labels included
        ties = T.tie_mask(doa, yd).reshape(B * S, 3 * nc)
        assert ties.sum() >= 2 and not got["ddoa_pre"][ties].any()


@pytest.mark.parametrize("mode", sorted(T.LOSS_MODES))
@pytest.mark.parametrize("B,S,nc", T.STRIDED_SHAPES)
def test_losses_strided_outputs(seld_lib, B, S, nc, mode):
    """the fused heads' shared gradient buffer: the same bits as dense rows, nothing written between or behind the two blocks"""
    data = T.loss_inputs(B, S, nc)
    dense = _Losses(seld_lib, *data, mode).run().results()
    strided = _Losses(seld_lib, *data, mode, strided=True).run().results()
    for k in T.TOL:
        _same_bits(f"losses {mode} {B, S, nc} {k} strided vs dense", strided[k], dense[k])


@pytest.mark.parametrize("mode", sorted(T.LOSS_MODES))
@pytest.mark.parametrize("B,S,nc", T.STRIDED_SHAPES)
def test_losses_deferred_finalize(seld_lib, B, S, nc, mode):
    """a training step's order: the gradients first, the scalars from the per-workgroup partials in a later launch"""
    data = T.loss_inputs(B, S, nc)
    now = _Losses(seld_lib, *data, mode).run().results()
    L = _Losses(seld_lib, *data, mode).run(defer=1)
    assert _all_nan_bits(L.sl.view), "the deferred call wrote sloss"
    if mode == "MMSE":
        assert _all_nan_bits(L.dl.view), "the deferred call wrote the MMSE dloss"
    later = L.finalize().results()
    for k in T.TOL:
        _same_bits(f"losses {mode} {B, S, nc} {k} deferred vs at once", later[k], now[k])
    again = L.run(defer=1).finalize().results()      # a second complete run on the same buffers
    for k in T.TOL:
        _same_bits(f"losses {mode} {B, S, nc} {k} second run", again[k], now[k])
    bare = _Losses(seld_lib, *data, mode, grads=False).run(defer=1).finalize().results()
    for k in ("sloss", "dloss"):
        _same_bits(f"losses {mode} {B, S, nc} {k} without gradients", bare[k], now[k])


def test_bce_clip_boundary(seld_lib):
    """p at, next to and beyond both clip bounds against y = 0, 1, 0.3: where the clip blocks the gradient it is exactly 0 (+0 or -0);
    elsewhere loss and gradient meet the bars against the float32-constant reference"""
    sed, ys, blocked = T.bce_boundary_case()
    doa = yd = np.zeros((1, 2, 36), np.float32)
    got = _Losses(seld_lib, sed, doa, ys, yd, "MSE").run().results()
    ref = T.losses_ref(sed, doa, ys, yd, "MSE")
    g = got["dsed_pre"].reshape(sed.shape)
    assert not g[blocked].any(), "a gradient passed the clip"
    assert g[~blocked].all() and np.array_equal(np.sign(g[~blocked]), np.sign(ref["dsed_pre"][~blocked]))
    _check_losses("BCE boundary", got, ref, keys=("sloss", "dsed_pre"))
    # each element alone at the bar, not only against the largest one of the set
    live = ~blocked
    e = np.abs(g[live] - ref["dsed_pre"][live]) / np.abs(ref["dsed_pre"][live])
    print(f"[parity] BCE boundary dsed_pre per element: worst {e.max():.3e}")
    assert e.max() <= T.TOL["dsed_pre"]


def test_fill_sets_the_given_mmse_denominator(seld_lib):
    """seld_m_losses with mmse_den > 0 puts it behind the scratch with fill_kernel: dloss and its gradient are the reference's with that one"""
    B, S, nc, den = 5, 13, 5, 2.5
    sed, doa, ys, yd = T.loss_inputs(B, S, nc)
    ins = [_in(sed), _in(doa), _in(ys), _in(yd)]
    sl, dl, gs, gd = _out(1, 1), _out(1, 1), _out(B * S, nc), _out(B * S, 3 * nc)
    scr = _out(1, int(seld_lib.seld_m_losses_scratch(B * S)))
    cfg = _cfg("MMSE", den)
    assert seld_lib.seld_m_losses(*[w.ptr() for w in ins], C.byref(cfg), sl.ptr(), dl.ptr(), gs.ptr(), gd.ptr(), scr.ptr(), B, S, nc, None) == 0
    torch.cuda.synchronize()
    ref = T.losses_ref(sed, doa, ys, yd, "MMSE", mmse_den=den)
    own = T.losses_ref(sed, doa, ys, yd, "MMSE")
    assert abs(ref["dloss"][0] / own["dloss"][0] - 1) > 0.5      # the labels' own denominator is far from 2.5: the two cannot be confused
    _check_losses(f"losses MMSE den={den}", {"sloss": sl.numpy(), "dloss": dl.numpy(), "dsed_pre": gs.numpy(), "ddoa_pre": gd.numpy()}, ref)
    assert scr.numpy().reshape(-1)[2 * B * S + 64] == np.float32(den)
    for w in ins:
        w.assert_unchanged("seld_m_losses")
    for w in (sl, dl, gs, gd, scr):
        w.assert_band("seld_m_losses")


# ------------------------------------------------------------------------------------------------ Adam, AGC
@pytest.mark.parametrize("step", T.ADAM_STEPS)
@pytest.mark.parametrize("n", T.ADAM_NS)
def test_adam_block_edges_and_late_steps(seld_lib, n, step):
    th, g, m, v, z = T.adam_case(n, step)
    wt, wg, wm, wv = _in(th, n), _in(g, n), _in(m, n), _in(v, n)
    assert seld_lib.seld_k_adam(wt.ptr(), wg.ptr(), wm.ptr(), wv.ptr(), n, 1e-3, 0.9, 0.999, 1e-7, step) == 0
    wg.assert_unchanged("adam g")
    for (name, w), r in zip((("theta", wt), ("m", wm), ("v", wv)), T.adam_ref(th, g, m, v, step)):
        w.assert_band(f"adam {name}")
        check(f"adam {name} n={n} step={step}", w.numpy().reshape(-1), r, tol=1e-6)
    _same_bits("adam theta where g = m = v = 0", wt.numpy().reshape(-1)[z], th[z])


@pytest.mark.parametrize("shape", T.AGC_SHAPES, ids=str)
def test_agc_one_variable(seld_lib, shape):
    """one variable at a non-zero offset of flat buffers: per unit against adaptive_clip_grad in float64, every unit compared"""
    th, g, clip = T.agc_case(shape)
    n = th.size
    wt, wg = _in(th, n), _Window(1, n, front=FRONT, back=BACK, data=g)      # FRONT > AGC_OFF: the flat buffers' bases lie inside the allocations
    base_t, base_g = C.c_void_p(wt.view.data_ptr() - 4 * T.AGC_OFF), C.c_void_p(wg.view.data_ptr() - 4 * T.AGC_OFF)
    assert seld_lib.seld_k_agc(base_t, base_g, T.AGC_OFF, len(shape), (C.c_int64 * 4)(*shape)) == 0
    wt.assert_unchanged("agc theta")
    wg.assert_band("agc g")
    got, ref = wg.numpy().reshape(shape), T.agc_ref(th, g)
    assert np.isfinite(got).all()
    rows, cols = T.agc_rows_cols(shape)
    kept = ~clip
    _same_bits("agc: units under their ceiling keep their bits", got.reshape(rows, cols)[:, kept], g.reshape(rows, cols)[:, kept])
    assert (got.reshape(rows, cols)[:, clip] != g.reshape(rows, cols)[:, clip]).any(axis=0).all(), "a unit above its ceiling was not clipped"
    e, tol = T.unit_err(got, ref), T.agc_tol(shape)
    print(f"[parity] agc {str(shape):20s} worst unit rel_err={e:.3e}  (bar {tol:.3e}, float32 CPU {T.unit_err(T.agc_f32(th, g), ref):.3e})")
    assert e <= tol


# ------------------------------------------------------------------------------------------------ the heads' tail
@pytest.mark.parametrize("act", [1, 2, 3])
@pytest.mark.parametrize("n", T.ACT_NS)
def test_act_bwd(seld_lib, n, act):
    y, dy = T.act_case(n, act)
    wy, wd = _in(y, n), _in(dy, n)
    assert seld_lib.seld_k_act_bwd(wy.ptr(), wd.ptr(), n, act) == 0
    wy.assert_unchanged("act_bwd y")
    wd.assert_band("act_bwd dy")
    got, ref = wd.numpy().reshape(-1), T.act_bwd_ref(y, dy, act)
    check(f"act_bwd act={act} n={n}", got, ref, tol=1e-6)
    assert not got[ref == 0].any()      # the activations' end values: exactly 0


@pytest.mark.parametrize("rows,nc", T.V1_SHAPES)
def test_v1_couple_fwd(seld_lib, rows, nc):
    sed, doa1, _, _ = T.v1_inputs(rows, nc)
    ws, wd = _in(sed), _in(doa1)
    o1, o2, o3 = _out(rows, 3 * nc), _out(rows, 3 * nc), _out(rows, 3 * nc)
    assert seld_lib.seld_k_v1_couple_fwd(ws.ptr(), wd.ptr(), o1.ptr(), o2.ptr(), rows, nc) == 0
    assert seld_lib.seld_k_v1_couple_fwd(ws.ptr(), wd.ptr(), o3.ptr(), None, rows, nc) == 0
    for w in (ws, wd):
        w.assert_unchanged("v1 fwd")
    for w in (o1, o2, o3):
        w.assert_band("v1 fwd")
    check(f"v1 fwd {rows, nc}", o1.numpy(), T.v1_fwd_ref(sed, doa1).reshape(rows, 3 * nc), tol=2e-6)
    _same_bits("v1 fwd out2", o2.numpy(), o1.numpy())
    _same_bits("v1 fwd without out2", o3.numpy(), o1.numpy())


@pytest.mark.parametrize("strided", [False, True], ids=["dense", "shared"])
@pytest.mark.parametrize("mode", sorted(T.LOSS_MODES))
@pytest.mark.parametrize("rows,nc", T.V1_SHAPES)
def test_v1_couple_bwd_behind_the_losses(seld_lib, rows, nc, mode, strided):
    """run_losses' order for seldnet_v1: the losses on (sed, coupled output) leave d / d(doa1 sed) in the DOA slot, the coupling's backward turns
    both slots into the gradients w.r.t. the two heads' pre-activations, in place"""
    sed, doa1, ys, yd = T.v1_inputs(rows, nc)
    ws, wd = _in(sed), _in(doa1)
    coupled = _out(rows, 3 * nc)
    assert seld_lib.seld_k_v1_couple_fwd(ws.ptr(), wd.ptr(), coupled.ptr(), None, rows, nc) == 0
    L = _Losses(seld_lib, sed, coupled.numpy().reshape(1, rows, 3 * nc), ys, yd, mode, strided=strided).run()
    ld_s, ld_d = (L.ld, L.ld) if strided else (nc, 3 * nc)
    assert seld_lib.seld_k_v1_couple_bwd(ws.ptr(), wd.ptr(), L.ps, ld_s, L.pd, ld_d, rows, nc) == 0
    for w in (ws, wd):
        w.assert_unchanged("v1 bwd")
    got, ref = L.results(), T.v1_bwd_ref(sed, doa1, ys, yd, mode)
    for k in ("dsed_pre", "ddoa_pre"):
        check(f"v1 bwd {mode} {rows, nc} {'shared' if strided else 'dense'} {k}", got[k].reshape(-1), ref[k].reshape(-1), tol=1e-4)


@pytest.mark.parametrize("ks", T.TIME_KS)
@pytest.mark.parametrize("B,S,Cc", T.TIME_SHAPES)
def test_time_expand_and_fold(seld_lib, B, S, Cc, ks):
    from oracle import seldnet_oracle as O
    x, dxe, prev = T.time_case(B, S, Cc, ks)
    wx, we = _in(x), _out(B * S, ks * Cc)
    assert seld_lib.seld_k_time_expand(wx.ptr(), we.ptr(), B, S, Cc, ks) == 0
    wx.assert_unchanged("time_expand x")
    we.assert_band("time_expand xe")
    xe = we.numpy().reshape(B, S, ks * Cc)
    _same_bits(f"time_expand {B, S, Cc} ks={ks}", xe, T.time_expand_ref(x, ks))
    K = np.random.default_rng(ks).standard_normal((ks, Cc, 6))
    check(f"time_expand @ kernel vs conv1d_same {B, S, Cc} ks={ks}", xe.astype(np.float64) @ K.reshape(ks * Cc, 6),
          O.conv1d_same(T.t64(x), T.t64(K), 0).numpy(), tol=1e-12)
    wdxe = _in(dxe)
    for accumulate in (0, 1):
        wdx = _Window(B * S, Cc, front=FRONT, back=BACK, data=prev) if accumulate else _out(B * S, Cc)
        assert seld_lib.seld_k_time_fold(wdxe.ptr(), wdx.ptr(), B, S, Cc, ks, accumulate) == 0
        wdxe.assert_unchanged("time_fold dxe")
        wdx.assert_band("time_fold dx")
        _same_bits(f"time_fold {B, S, Cc} ks={ks} accumulate={accumulate}", wdx.numpy().reshape(B, S, Cc),
                   T.time_fold_ref(dxe, ks, prev if accumulate else None))


@pytest.mark.parametrize("layer,step", T.DROP_STREAMS)
@pytest.mark.parametrize("rate", T.DROP_RATES)
@pytest.mark.parametrize("n", T.DROP_NS)
def test_dropout4(seld_lib, n, rate, layer, step):
    v = np.random.default_rng(n).standard_normal(n).astype(np.float32)
    keep, ref = T.dropout4_ref(v, rate, T.DROP_SEED, layer, step)
    wi, wo = _in(v, n), _out(1, n)
    args = (n, rate, C.c_uint64(T.DROP_SEED), layer, step)
    assert seld_lib.seld_k_dropout4(wi.ptr(), wo.ptr(), *args) == 0
    wi.assert_unchanged("dropout4 in")
    wo.assert_band("dropout4 out")
    got = wo.numpy().reshape(-1)
    assert np.array_equal(got != 0, keep & (v != 0)), "the mask is not philox_uniform(...) >= float32(rate)"
    _same_bits(f"dropout4 n={n} rate={rate}", got, ref)
    if rate == 0.0:
        _same_bits("dropout4 rate 0 is the identity", got, v)
    assert seld_lib.seld_k_dropout4(wi.ptr(), wi.ptr(), *args) == 0      # in place, as the backward pass runs it
    wi.assert_band("dropout4 in place")
    _same_bits(f"dropout4 n={n} rate={rate} in place", wi.numpy().reshape(-1), ref)


@pytest.mark.parametrize("rows,S,F", T.MASK_SHAPES)
def test_mask_rows(seld_lib, rows, S, F):
    x, mask, prev = T.mask_rows_case(rows, S, F)
    wx, wm = _in(x), _in(mask)
    wo, wa = _out(rows, F), _Window(rows, F, front=FRONT, back=BACK, data=prev)
    assert seld_lib.seld_k_mask_rows(wx.ptr(), wm.ptr(), wo.ptr(), rows, S, F, 0) == 0
    assert seld_lib.seld_k_mask_rows(wx.ptr(), wm.ptr(), wa.ptr(), rows, S, F, 1) == 0
    for w in (wx, wm):
        w.assert_unchanged("mask_rows")
    for w in (wo, wa):
        w.assert_band("mask_rows")
    _same_bits(f"mask_rows {rows, S, F}", wo.numpy(), T.mask_rows_ref(x, mask, S, dtype=np.float32))
    check(f"mask_rows accumulate {rows, S, F}", wa.numpy(), T.mask_rows_ref(x, mask, S, prev), tol=1e-6)
