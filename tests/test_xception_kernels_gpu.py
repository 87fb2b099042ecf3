"""xception_block's kernels one by one (seld_amd/csrc/xception.hip through the seld_k_xc_* entry points) against the float64 reference of
tests/xception_oracle.py, at the tile and grid edges of each kernel.  Every output buffer is NaN-filled and carved out of a larger allocation with
GUARD sentinel floats on both sides, asserted unchanged afterwards (a partial tile must not write past its tensor); wherever a ReLU gate or the
folded BatchNormalization (`aff`) enters, the inputs are first moved to min |x scale + shift| >= 1e-4 (float64), where no fp32 evaluation takes a
gate differently, so no element is excluded from any comparison.  Beside every kernel error the error of plain torch fp32 on the CPU is printed."""
import functools

import numpy as np
import pytest
import torch

import xception_oracle as X
from helpers import check, dev, ptr, rel_err

pytestmark = pytest.mark.gpu

GUARD = 1024
SENTINEL = 123456.0
EW = X.ELEMENTWISE_BAR


class Guarded:
    """NaN-filled output tensors inside one allocation each, GUARD sentinel floats before and behind"""

    def __init__(self):
        self.bufs = []

    def out(self, *shape):
        n = int(np.prod(shape))
        whole = torch.full((n + 2 * GUARD,), SENTINEL, device="cuda")
        whole[GUARD:GUARD + n] = float("nan")
        self.bufs.append((whole, n))
        return whole[GUARD:GUARD + n].view(*shape)

    def assert_intact(self):
        for whole, n in self.bufs:
            assert bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[GUARD + n:] == SENTINEL).all()), "a kernel wrote outside its output tensor"


def p_(t):
    return ptr(t) if t is not None else None


def ew(name, got, ref, ref32):
    """an elementwise fp32 output: finite, within EW of the float64 reference over its maximum; the fp32 CPU reference's own error beside it"""
    got, ref = np.asarray(got), np.asarray(ref)
    e, e32 = rel_err(got, ref), rel_err(np.asarray(ref32), ref)
    print(f"[xc] {name:44s} kernel {e:.3e}   fp32 cpu {e32:.3e}   (|ref|max={np.abs(ref).max():.3e})")
    assert np.isfinite(got).all(), f"{name}: non-finite output"
    assert e <= EW, f"{name}: rel err {e:.3e} > {EW}"
    return e


def signed_sum(name, got, ref, terms):
    """a per-channel sum of signed terms: error over max_c sum |term| (fp32 accumulation is bounded relative to that, not to the cancelled sum)"""
    e = X.rel_err_abs_sum(got, ref, terms)
    print(f"[xc] {name:44s} kernel {e:.3e}   (over max_c sum|term|)")
    assert np.isfinite(np.asarray(got)).all(), f"{name}: non-finite output"
    assert e <= 1e-4, f"{name}: err {e:.3e} > 1e-4"


@pytest.fixture
def options(seld_lib):
    """seld_k_set_option, every option back at its default afterwards"""
    def set_(**kv):
        for k, v in kv.items():
            assert seld_lib.seld_k_set_option(k.encode(), v) == 0
    try:
        yield set_
    finally:
        seld_lib.seld_k_set_option(b"xc_w16", 1)
        seld_lib.seld_k_set_option(b"xc_xcd_map", 1)


# ---------------------------------------------------------------------------------------------- depthwise forward
@functools.lru_cache(maxsize=None)
def _dw_case(B, H, W, with_aff):
    x, k, _, aff = X.unit_inputs(B, H, W)
    aff = aff if with_aff else None
    x, _ = X.apply_gate_margin(x, aff)
    return x, k, aff, X.depthwise_forward(x, k, aff).numpy(), X.depthwise_forward(x, k, aff, torch.float32).numpy()


@pytest.mark.parametrize("with_aff", [1, 0])
@pytest.mark.parametrize("B,H,W", X.DW_FWD_W16 + X.DW_FWD_GENERIC)
def test_depthwise_forward(seld_lib, options, B, H, W, with_aff):
    """dw3x3_w16_kernel and the generic dw3x3_kernel, forward, with and without the folded BatchNormalization, under both block maps: every
    form against float64, and at W = 16 the four choices bit for bit against each other ("the same taps in the same order, the same fmaf")"""
    x, k, aff, ref, ref32 = _dw_case(B, H, W, with_aff)
    assert X.gate_margin(x, aff) >= X.GATE_MARGIN
    xd, kd, ad = dev(x), dev(k), dev(aff) if aff is not None else None
    outs = {}
    for w16 in ((1, 0) if W == 16 else (0,)):
        for xcd in (1, 0):
            options(xc_w16=w16, xc_xcd_map=xcd)
            g = Guarded()
            y = g.out(B, H, W, 64)
            assert seld_lib.seld_k_xc_dw_fwd(ptr(xd), ptr(kd), p_(ad), ptr(y), B, H, W) == 0
            g.assert_intact()
            outs[w16, xcd] = y.cpu().numpy()
            ew(f"dw fwd {B, H, W} aff={with_aff} w16={w16} xcd={xcd}", outs[w16, xcd], ref, ref32)
    first = next(iter(outs.values()))
    for key, o in outs.items():
        assert np.array_equal(o.view(np.int32), first.view(np.int32)), f"choice {key} differs in bits"


# ---------------------------------------------------------------------------------------------- unit forward
@functools.lru_cache(maxsize=2)
def _unit_case(B, H, with_aff):
    x, k, wpw, aff = X.unit_inputs(B, H)
    aff = aff if with_aff else None
    x, _ = X.apply_gate_margin(x, aff)
    ref = [t.numpy() for t in X.unit_forward(x, k, wpw, aff)]
    ref32 = [t.numpy() for t in X.unit_forward(x, k, wpw, aff, torch.float32)[:2]]
    return x, k, wpw, aff, ref, ref32


def _run_unit(seld_lib, case, B, H, fused, want_sums, tag):
    x, k, wpw, aff, (dwo_r, z_r, s1_r, s2_r), (dwo32, z32) = case
    g = Guarded()
    dwo, z, sums = g.out(B, H, 16, 64), g.out(B, H, 16, 64), g.out(128)
    xd, kd, wd, ad = dev(x), dev(k), dev(wpw), dev(aff) if aff is not None else None      # alive until the call returns
    rc = seld_lib.seld_k_xc_unit_fwd(ptr(xd), ptr(kd), ptr(wd), p_(ad), ptr(dwo), ptr(z), ptr(sums) if want_sums else None, B, H, fused)
    assert rc == 0
    g.assert_intact()
    dwo, z, sums = dwo.cpu().numpy(), z.cpu().numpy(), sums.cpu().numpy()
    ew(f"unit fwd {tag} dwo", dwo, dwo_r, dwo32)
    ew(f"unit fwd {tag} z", z, z_r, z32)
    if want_sums:
        signed_sum(f"unit fwd {tag} sum z", sums[:64], s1_r, z_r)
        check(f"unit fwd {tag} sum z^2", sums[64:], s2_r)
    else:
        assert np.isnan(sums).all()      # not asked for: not written
    return dwo, z, sums


@pytest.mark.parametrize("with_aff", [1, 0])
@pytest.mark.parametrize("B,H", X.UNIT_SHAPES)
def test_unit_forward(seld_lib, B, H, with_aff):
    """xc_unit_fwd_kernel (fused = 1) and the three-kernel route (fused = 0), with and without statistics: dwo, z, sum z, sum z^2.  One row, one
    partial tile, exact tiles with an image boundary between them, 8 + 1 rows, several tiles per image"""
    case = _unit_case(B, H, with_aff)
    assert X.gate_margin(case[0], case[3]) >= X.GATE_MARGIN
    for fused in (1, 0):
        for want_sums in (1, 0):
            _run_unit(seld_lib, case, B, H, fused, want_sums, f"{B, H} aff={with_aff} fused={fused} sums={want_sums}")


def test_unit_forward_more_tiles_than_workgroups(seld_lib):
    """(260, 25): 1040 tiles on the 512 persistent workgroups — workgroups walk two and three tiles (prefetch, commit, and the last tile's
    re-read of itself), the last tile of every image holds ONE valid row (the statistics must not count the other seven).  Twice: the reductions
    are fixed-order, so the bits repeat"""
    B, H = X.UNIT_BIG
    case = _unit_case(B, H, 1)
    assert X.gate_margin(case[0], case[3]) >= X.GATE_MARGIN
    a = _run_unit(seld_lib, case, B, H, 1, 1, f"{B, H} aff=1 fused=1 sums=1")
    b = _run_unit(seld_lib, case, B, H, 1, 1, f"{B, H} again")
    for u, v, n in zip(a, b, ("dwo", "z", "sums")):
        assert np.array_equal(u.view(np.int32), v.view(np.int32)), f"{n}: two runs differ in bits"


# ---------------------------------------------------------------------------------------------- pointwise backward
@functools.lru_cache(maxsize=2)
def _pw_case(npix):
    rng = np.random.default_rng(npix)
    dwo = rng.standard_normal((npix, 64)).astype(np.float32)
    gy = rng.standard_normal((npix, 64)).astype(np.float32)
    wpw = (rng.standard_normal((64, 64)) / 8).astype(np.float32)
    gamma = (1.0 + 0.5 * rng.standard_normal(64)).astype(np.float32)
    gamma[[3, 17, 40]] = [-0.7, -1.2, -0.4]
    r = X.pw_backward(dwo, wpw, gamma, gy)
    r32 = X.pw_backward(dwo, wpw, gamma, gy, torch.float32)
    f32 = lambda t: t.numpy().astype(np.float32)
    # what the model would hold: the float64 values of the same batch rounded to fp32
    held = dict(z=f32(r["z"]), mean=f32(r["mean"]), invstd=f32(r["invstd"]), scale=f32(X.T(gamma) * r["invstd"]),
                c1c2=np.concatenate([f32(r["c1"]), f32(r["c2"])]))
    return dwo, gy, wpw, held, r["f1"].numpy(), r["dw"].numpy(), r32["f1"].numpy(), r32["dw"].numpy()


@pytest.mark.parametrize("npix", X.PW_NPIX)
def test_pointwise_backward(seld_lib, npix):
    """xc_pw_bwd_kernel + the one-stage (mode 1) and two-stage (mode 2) slab combine, and the three-kernel route (mode 0): f1 = dz W^T and
    dW = dwo^T dz with dz = BatchNorm'(gy) formed on load, against autograd through BatchNorm(training)(dwo W) in float64.  npix around the
    128-pixel tile (tail pixels must add nothing to dW), and more than 1024 tiles on the 512 workgroups"""
    dwo, gy, wpw, held, f1_r, dw_r, f1_32, dw_32 = _pw_case(npix)
    d = {n: dev(v) for n, v in held.items()}
    dwod, gyd, wd = dev(dwo), dev(gy), dev(wpw)
    for mode in ((1, 2) if npix == X.PW_NPIX_FUSED_ONLY else (1, 2, 0)):
        g = Guarded()
        f1, dw = g.out(npix, 64), g.out(64, 64)
        rc = seld_lib.seld_k_xc_pw_bwd(ptr(d["z"]), ptr(gyd), ptr(dwod), ptr(wd), ptr(d["mean"]), ptr(d["invstd"]), ptr(d["scale"]), ptr(d["c1c2"]),
                                       ptr(f1), ptr(dw), npix, mode)
        assert rc == 0
        g.assert_intact()
        ew(f"pw bwd npix={npix} mode={mode} f1", f1.cpu().numpy(), f1_r, f1_32)
        print(f"[xc] pw bwd npix={npix} dw: fp32 cpu {rel_err(dw_32, dw_r):.3e}")
        check(f"pw bwd npix={npix} mode={mode} dw", dw.cpu().numpy(), dw_r)


# ---------------------------------------------------------------------------------------------- BatchNorm kernels
def _bn_inputs(npix):
    rng = np.random.default_rng(7 * npix + 1)
    z = rng.standard_normal((npix, 64)).astype(np.float32)
    dy = rng.standard_normal((npix, 64)).astype(np.float32)
    res = rng.standard_normal((npix, 64)).astype(np.float32)
    scale = (1.0 + 0.5 * rng.standard_normal(64)).astype(np.float32)
    scale[[3, 17, 40]] = [-0.7, -1.2, -0.4]
    shift = (0.3 * rng.standard_normal(64)).astype(np.float32)
    return z, dy, res, scale, shift


@pytest.mark.parametrize("npix", X.BN_NPIX)
def test_bn_stats(seld_lib, npix):
    """xc_reduce_kernel<false> + combine: [sum z | sum z^2]; 16 pixels per workgroup pass, beyond 512 workgroups the strided second pass"""
    z = _bn_inputs(npix)[0]
    s1, s2 = X.bn_stats(z)
    g = Guarded()
    sums = g.out(128)
    zd = dev(z)
    assert seld_lib.seld_k_xc_bn_stats(ptr(zd), ptr(sums), npix) == 0
    g.assert_intact()
    sums = sums.cpu().numpy()
    signed_sum(f"bn stats npix={npix} sum z", sums[:64], s1.numpy(), z)
    check(f"bn stats npix={npix} sum z^2", sums[64:], s2.numpy())


@pytest.mark.parametrize("with_res", [1, 0])
@pytest.mark.parametrize("npix", X.BN_NPIX)
def test_bn_apply(seld_lib, npix, with_res):
    """out = z scale + shift (+ res)"""
    z, _, res, scale, shift = _bn_inputs(npix)
    res = res if with_res else None
    g = Guarded()
    out = g.out(npix, 64)
    zd, scd, shd, rd = dev(z), dev(scale), dev(shift), dev(res) if with_res else None
    assert seld_lib.seld_k_xc_bn_apply(ptr(zd), ptr(scd), ptr(shd), p_(rd), ptr(out), npix) == 0
    g.assert_intact()
    ew(f"bn apply npix={npix} res={with_res}", out.cpu().numpy(), X.bn_apply(z, scale, shift, res).numpy(),
       X.bn_apply(z, scale, shift, res, torch.float32).numpy())


@pytest.mark.parametrize("npix", X.BN_NPIX)
def test_bn_backward(seld_lib, npix):
    """xc_reduce_kernel<true>, bn_bwd_finalize, xc_bn_bwd_dz: dz, dgamma, dbeta and c1c2 against autograd through BatchNorm(training)(z) in
    float64; mean / invstd / scale = gamma invstd are the float64 values of the same batch rounded to fp32"""
    z, dy, _, gamma, _ = _bn_inputs(npix)
    r = X.bn_backward(z, dy, gamma)
    r32 = X.bn_backward(z, dy, gamma, torch.float32)
    f32 = lambda t: t.numpy().astype(np.float32)
    g = Guarded()
    dz, dg, db, c1c2 = g.out(npix, 64), g.out(64), g.out(64), g.out(128)
    zd, dyd, md, isd, scd = dev(z), dev(dy), dev(f32(r["mean"])), dev(f32(r["invstd"])), dev(f32(X.T(gamma) * r["invstd"]))
    rc = seld_lib.seld_k_xc_bn_bwd(ptr(zd), ptr(dyd), ptr(md), ptr(isd), ptr(scd), ptr(dz), ptr(dg), ptr(db), ptr(c1c2), npix)
    assert rc == 0
    g.assert_intact()
    ew(f"bn bwd npix={npix} dz", dz.cpu().numpy(), r["dz"].numpy(), r32["dz"].numpy())
    check(f"bn bwd npix={npix} dgamma", dg.cpu().numpy(), r["dgamma"].numpy())
    signed_sum(f"bn bwd npix={npix} dbeta", db.cpu().numpy(), r["dbeta"].numpy(), dy)
    c = c1c2.cpu().numpy()
    signed_sum(f"bn bwd npix={npix} c1", c[:64], r["c1"].numpy(), dy / npix)
    check(f"bn bwd npix={npix} c2", c[64:], r["c2"].numpy())
