"""The 64 -> 64 3x3 convolution family (conv_sb.hip, conv_wgrad_sb.hip, the 64 -> 64 kernels of conv.hip), each kernel form called through its
seld_k_* entry point over the edge table (B = 3, H in {1, 2, R - 1, R, R + 1, 2 R + 1} for the form's R-row tiles) and over a shape of more than
twice the launcher's grid cap in tiles, and compared with a plain fp64 statement of the operation.  Cases, inputs, references and bars are in
tests/conv64_cases.py; tests/test_conv64_family_cpu.py holds what the cases promise.

Every operand and output lies between two guard bands of 16 384 floats (a tile's rows at the least) filled with a finite canary; outputs are
NaN-filled.  After a launch the output holds no NaN, the canaries and the inputs hold their bits, and a second launch gives the same bits (no kernel
of the family uses atomics).  A refused call leaves every output as it was.  Options are restored in `finally`.

kernel -> instantiation <WLOG2, R, STATS, ONE, FOUR, PRE, EXT> -> launcher -> test [case ids]
  conv64_fwd_sbd_kernel
    <4,16,S,0>, <3,32,S,0>, <2,48,S,0>   launch_sbd, S = false / true            test_forward [six-W16 / W8 / W4] (both S);  S = false also
                                                                                 test_input_gradient [six-W16 / W8 / W4]
    <4,16,S,1>, <2,48,S,1>               launch_sbd under bf16_single            test_forward [one-W16, one-W4] (both S), test_input_gradient [one-W16]
    <3,32,S,1>                           launch_sbd under bf16_single            test_kernels_gpu.py::test_bf16_single_product_conv64 (kept)
    <4,16,0,0,FOUR>                      launch_sbd, dgrad_r8 = 0                test_input_gradient [four-R16-W16], test_four_product_tilings_same_bits
    <4,8,0,0,FOUR>                       launch_sbd_four, dgrad_r8 = 1           test_input_gradient [four-R8-W16], test_four_product_tilings_same_bits
    <2,48,0,0,FOUR>, <3,32,0,0,FOUR>     launch_sbd                              test_input_gradient [four-W4, four-W8]
    <4,16,S,0,0,PRE>, <2,48,S,0,0,PRE>   launch_sbd with pre_scale               test_pre_ext [W16-*, W4-*] (both S, with and without pre_out)
    <4,16,S,0,0,PRE,EXT>                 launch_sbd with pre_scale and ext_out   test_pre_ext [W16-*] (both S, with and without pre_out)
    the launchers' refusals                                                      test_pre_ext_refusals
  conv64_fwd_sb_kernel<S>                conv64_sb, every other width            test_forward [generic-W32, generic-W2] (both S), test_input_gradient [six-W32, six-W2] (S = false)
  split_weights_batch_kernel             flip 0 / flip 1                         every forward / input-gradient test above
  conv64_fwd_kernel<S>                   launch_conv64_fwd (conv64_split_bf16 = 0)   test_forward [f32-W16, f32-W32] (both S), test_input_gradient [f32-*] (S = false)
  conv64_wgrad_sb_kernel<L, false>, <L, true>, <L, false, true>, L = 4, 3, 2     test_kernel_gradient [six- / one- / four-W16, W8, W4]
  conv64_wgrad_kernel<1 .. 5>            launch_conv64_wgrad                     test_kernel_gradient [f32-W2, W4, W8, W16, W32]: the W = 32 and W = 2 shapes that
                                                                                 test_kernels_gpu.py::test_conv_wgrad does not have are here

The hand-made faults the file was tried against are in DESIGN.md 3aa."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import conv64_cases as K
import helpers
from conv64_cases import FORMS, mag_err, report, report_exact

pytestmark = pytest.mark.gpu

GUARD = 16384                       # floats in front of and behind every tensor: the largest tile here is 256 pixels x 64 channels
CANARY = 0x4B1D5EED                 # a finite float (1.03e7): a kernel that reads a guard computes with it, one that writes it is seen
UNSUPPORTED = -2
assert all(f.R * f.W * K.C <= GUARD for f in FORMS.values() if f.name.startswith(("sbd", "sb", "f32")))


def _bits(t):
    return t.view(torch.int32)


class Buf:
    """a tensor of `shape` between two guard bands; an output when data is None (NaN-filled)"""

    def __init__(self, shape, data=None):
        self.shape, self.n = tuple(shape), int(np.prod(shape))
        self.buf = torch.empty(GUARD + self.n + GUARD, device="cuda")
        _bits(self.buf).fill_(CANARY)
        self.body = self.buf[GUARD:GUARD + self.n]
        if data is None:
            self.body.fill_(float("nan"))
        else:
            self.body.copy_(helpers.dev(np.asarray(data, np.float32).reshape(-1)))      # a copy: the shared inputs are read-only
        self.saved = _bits(self.buf).clone()

    def ptr(self):
        return C.c_void_p(self.body.data_ptr())

    def unchanged(self):
        return torch.equal(_bits(self.buf), self.saved)

    def freeze(self):
        """an output that now serves as an input"""
        self.saved = _bits(self.buf).clone()
        return self

    def guards_ok(self):
        b = _bits(self.buf)
        return bool((b[:GUARD] == CANARY).all()) and bool((b[GUARD + self.n:] == CANARY).all())

    def written(self):
        return not bool(torch.isnan(self.body).any())

    def numpy(self):
        return self.body.cpu().numpy().reshape(self.shape)


def P(x):
    return None if x is None else x.ptr()


def settle(name, ins, outs):
    torch.cuda.synchronize()
    for i, b in enumerate(ins):
        assert b is None or b.unchanged(), f"{name}: input {i}, or a guard band around it, was written"
    for i, b in enumerate(outs):
        if b is not None:
            assert b.guards_ok(), f"{name}: a float outside output {i} was written"
            assert b.written(), f"{name}: output {i} holds a NaN"


def same_bits(name, a, b):
    for i, (u, v) in enumerate(zip(a, b)):
        if u is not None:
            assert torch.equal(_bits(u.buf), _bits(v.buf)), f"{name}: output {i} differs"


def twice(name, run):
    """run() makes fresh outputs, launches and returns them: two launches give the same bits"""
    a, b = run(), run()
    same_bits(name + " (second launch)", a, b)
    return a


@contextlib.contextmanager
def options(lib, **kw):
    try:
        for k, v in kw.items():
            assert lib.seld_k_set_option(k.encode(), v) == 0
        yield
    finally:
        for k, v in K.DEFAULTS.items():
            lib.seld_k_set_option(k.encode(), v)


@functools.lru_cache(maxsize=None)
def dev_weights():
    w, bias, wd = K.weights()
    return Buf(w.shape, w), Buf(bias.shape, bias), Buf(wd.shape, wd)


@functools.lru_cache(maxsize=8)
def dev_images(B, H, W):
    x, dz = K.images(B, H, W)
    return Buf(x.shape, x), Buf(dz.shape, dz)


def check_mag(name, got, ref, mag, bar):
    helpers.check(name, got, ref)
    report(name + " / magnitude", mag_err(got, ref, mag), bar)


def check_stats(name, st, zgot):
    sref, smag = K.stats_ref(zgot)
    s = st.numpy()
    helpers.check(name + " sum", s[:64], sref[:64])
    helpers.check(name + " sum of squares", s[64:], sref[64:])
    report(name + " / magnitude", mag_err(s, sref, smag), K.BAR6)


def _ids(cases):
    return [f"{fid}-B{B}-H{H}" for fid, B, H in cases]


# ================================================================ forward
FWD = K.cases(K.FWD_FORMS)


@pytest.mark.parametrize("fid,B,H", FWD, ids=_ids(FWD))
def test_forward(seld_lib, fid, B, H):
    _, tf, opts, kind, bar = K.form_of(K.FWD_FORMS, fid)
    W = FORMS[tf].W
    x, _ = dev_images(B, H, W)
    w, bias, _ = dev_weights()
    ref, mag = K.with_bias(*K.fwd_ref(kind, B, H, W))
    with options(seld_lib, **opts):
        for stats in (False, True):
            name = f"conv64 fwd {fid} {B, H} stats={int(stats)}"

            def run():
                z, st = Buf((B, H, W, 64)), Buf((128,)) if stats else None
                assert seld_lib.seld_k_conv3x3_fwd(P(x), P(w), P(bias), P(z), P(st), B, H, W, 64, 64) == 0
                settle(name, (x, w, bias), (z, st))
                return z, st
            z, st = twice(name, run)
            zg = z.numpy()
            check_mag(name, zg, ref, mag, bar)
            if stats:
                check_stats(name + " stats", st, zg)


# ================================================================ input gradient
DGRAD = K.cases(K.DGRAD_FORMS)


def _dgrad(lib, name, x, wd, B, H, W):
    def run():
        dx = Buf((B, H, W, 64))
        assert lib.seld_k_conv3x3_dgrad(P(x), P(wd), P(dx), B, H, W, 64, 64) == 0
        settle(name, (x, wd), (dx,))
        return (dx,)
    return twice(name, run)[0]


@pytest.mark.parametrize("fid,B,H", DGRAD, ids=_ids(DGRAD))
def test_input_gradient(seld_lib, fid, B, H):
    """dz = the case's image, the kernel = weights()[2], whose input gradient is the convolution with weights()[0]: the forward's reference"""
    _, tf, opts, kind, bar = K.form_of(K.DGRAD_FORMS, fid)
    W = FORMS[tf].W
    x, _ = dev_images(B, H, W)
    wd = dev_weights()[2]
    ref, mag = K.fwd_ref(kind, B, H, W)
    with options(seld_lib, **opts):
        dx = _dgrad(seld_lib, f"conv64 dgrad {fid} {B, H}", x, wd, B, H, W)
    check_mag(f"conv64 dgrad {fid} {B, H}", dx.numpy(), ref, mag, bar)


FOUR_SHAPES = sorted(set(K.shapes("sbd16")) | set(K.shapes("sbd_four16")))


@pytest.mark.parametrize("B,H", FOUR_SHAPES, ids=[f"B{B}-H{H}" for B, H in FOUR_SHAPES])
def test_four_product_tilings_same_bits(seld_lib, B, H):
    """common.h KernelChoices::dgrad_r8: "the same bits" on 8-row tiles (launch_sbd_four<4, 8>) and on 16-row tiles (launch_sbd<4, 16>)"""
    x, _ = dev_images(B, H, 16)
    wd = dev_weights()[2]
    out = []
    for r8 in (0, 1):
        with options(seld_lib, dgrad_r8=r8):
            out.append(_dgrad(seld_lib, f"conv64 dgrad four r8={r8} {B, H}", x, wd, B, H, 16))
    same_bits(f"conv64 dgrad four, 16-row against 8-row tiles {B, H}", out[:1], out[1:])


# ================================================================ kernel and bias gradient
WGRAD = K.cases(K.WGRAD_FORMS)


@pytest.mark.parametrize("fid,B,H", WGRAD, ids=_ids(WGRAD))
def test_kernel_gradient(seld_lib, fid, B, H):
    _, tf, opts, kind, bar = K.form_of(K.WGRAD_FORMS, fid)
    W = FORMS[tf].W
    x, dz = dev_images(B, H, W)
    dwr, mw, dbr, mb = K.wgrad_ref(kind, B, H, W)
    name = f"conv64 wgrad {fid} {B, H}"
    with options(seld_lib, **opts):
        def run():
            dw, db = Buf((9, 64, 64)), Buf((64,))
            assert seld_lib.seld_k_conv3x3_wgrad(P(x), P(dz), P(dw), P(db), B, H, W, 64, 64) == 0
            settle(name, (x, dz), (dw, db))
            return dw, db
        dw, db = twice(name, run)
    check_mag(name + " dw", dw.numpy(), dwr, mw, bar)
    check_mag(name + " db", db.numpy(), dbr, mb, K.BAR6)      # the bias gradient sums the unsplit dz in every form


# ================================================================ PRE / EXT
PRE = [(W, B, H) for W in K.PRE_WIDTHS for B, H in K.shapes(f"sbd{W}")]


@pytest.mark.parametrize("W,B,H", PRE, ids=[f"W{W}-B{B}-H{H}" for W, B, H in PRE])
def test_pre_ext(seld_lib, W, B, H):
    """seld_k_conv3x3_fwd_pre: BatchNorm + ReLU of the previous block on load (PRE), the activated rows to pre_out, the (1, 4) windows' extremes to
    ext_out (EXT, W = 16) — against the stand-alone passes bit for bit and against the fp64 convolution of the float32 activation"""
    lib = seld_lib
    xe, _ = dev_images(B, H, W)
    w, bias, _ = dev_weights()
    scale, shift, gamma, scale2, shift2 = (Buf(a.shape, a) for a in K.pre_params())
    act = K.activated(B, H, W)
    n = B * H * W * 64
    name = f"conv64 pre W{W} {B, H}"
    # the stand-alone passes: the activation, and the plain convolution of it
    a = Buf((B, H, W, 64))
    assert lib.seld_k_bn_relu_ext(P(xe), P(scale), P(shift), P(a), n) == 0
    settle(name + " bn_relu_ext", (xe, scale, shift), (a,))
    report_exact(name + " bn_relu_ext against the float32 restatement", a.numpy(), act)
    a_in = Buf((B, H, W, 64), a.numpy())
    plain = {}
    for stats in (False, True):
        z0, st0 = Buf((B, H, W, 64)), Buf((128,)) if stats else None
        assert lib.seld_k_conv3x3_fwd(P(a_in), P(w), P(bias), P(z0), P(st0), B, H, W, 64, 64) == 0
        settle(name + " plain", (a_in, w, bias), (z0, st0))
        plain[stats] = (z0, st0)
    ref, mag = K.with_bias(*K.fwd_ref("act", B, H, W))
    for stats in (False, True):
        for keep in (True, False):
            for ext in ((False, True) if W == 16 else (False,)):
                nm = f"{name} stats={int(stats)} pre_out={int(keep)} ext={int(ext)}"

                def run():
                    z, st = Buf((B, H, W, 64)), Buf((128,)) if stats else None
                    po = Buf((B, H, W, 64)) if keep else None
                    eo = Buf((B, H, W // 4, 64)) if ext else None
                    assert lib.seld_k_conv3x3_fwd_pre(P(xe), P(scale), P(shift), P(w), P(bias), P(z), P(st), P(po), P(gamma) if ext else None, P(eo), B, H, W) == 0
                    settle(nm, (xe, scale, shift, w, bias, gamma), (z, st, po, eo))
                    return z, st, po, eo
                z, st, po, eo = twice(nm, run)
                zg = z.numpy()
                report_exact(nm + " z against conv3x3_fwd of the activation", zg, plain[stats][0].numpy())
                if stats:
                    report_exact(nm + " stats against conv3x3_fwd's", st.numpy(), plain[True][1].numpy())
                if keep:
                    report_exact(nm + " pre_out against the float32 restatement", po.numpy(), act)
                    report_exact(nm + " pre_out against bn_relu_ext", po.numpy(), a.numpy())
                if ext:
                    report_exact(nm + " ext_out against the selection over z", eo.numpy(), K.ext_select(zg, K.pre_params()[2]))
                    p1, p2 = Buf((B, H, W // 4, 64)), Buf((B, H, W // 4, 64))
                    eo.freeze(), z.freeze()
                    assert lib.seld_k_bn_relu_ext(P(eo), P(scale2), P(shift2), P(p1), n // 4) == 0
                    assert lib.seld_k_bn_relu_pool_fwd(P(z), P(scale2), P(shift2), P(p2), B, H, W, 64, 1, 4) == 0
                    settle(nm + " pooled", (eo, z, scale2, shift2), (p1, p2))
                    report_exact(nm + " bn_relu_ext(ext_out) against bn_relu_pool_fwd(z)", p1.numpy(), p2.numpy())
    check_mag(name + " z", plain[False][0].numpy(), ref, mag, K.BAR6)      # the same bits as every PRE form's z, by the comparisons above


@pytest.mark.parametrize("what,kw", K.PRE_REFUSALS, ids=[r[0] for r in K.PRE_REFUSALS])
def test_pre_ext_refusals(seld_lib, what, kw):
    lib = seld_lib
    assert K.fwd_pre_refuses(**kw)
    W, B, H = kw["W"], 3, 2
    x, _ = dev_images(B, H, W)
    w, bias, _ = dev_weights()
    scale, shift, gamma = (Buf(a.shape, a) for a in K.pre_params()[:3])
    z, st, po = Buf((B, H, W, 64)), Buf((128,)), Buf((B, H, W, 64))
    eo = Buf((B, H, max(W // 4, 1), 64)) if kw.get("ext") else None
    pre = kw.get("pre", True)
    with options(lib, bf16_single=int(kw.get("single", False))):
        rc = lib.seld_k_conv3x3_fwd_pre(P(x), P(scale) if pre else None, P(shift) if pre else None, P(w), P(bias), P(z), P(st),
                                        P(x) if kw.get("pre_out_is_x") else P(po), P(gamma) if kw.get("ext_gamma", True) and eo is not None else None, P(eo), B, H, W)
    torch.cuda.synchronize()
    assert rc == UNSUPPORTED, f"{what}: returned {rc}"
    for i, b in enumerate((x, z, st, po, eo)):
        assert b is None or b.unchanged(), f"{what}: the refused call wrote tensor {i}"
    # what it refuses runs without the refused part
    if pre and W in K.PRE_WIDTHS:
        z2 = Buf((B, H, W, 64))
        assert lib.seld_k_conv3x3_fwd_pre(P(x), P(scale), P(shift), P(w), P(bias), P(z2), None, P(po), None, None, B, H, W) == 0
        settle(what + " (accepted form)", (x,), (z2, po))
