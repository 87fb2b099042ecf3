"""The GEMM family (gemm.hip, gemm_sb.hip, gemm_tn_sb.hip, prep.hip), each kernel form called through the seld_k_*_ex entry points with the
arguments the train step passes — leading dimensions, modes, epilogues, split limits, jobs — and compared with a plain fp64 statement of the
operation.  Cases, inputs, references and the bars are in tests/gemm_cases.py; tests/test_gemm_family_cpu.py holds what the cases promise.

Every operand and output is a window inside a NaN-filled allocation (the _Window of test_attention_gpu.py): after a call the floats around an
output and in the padding columns of its rows still hold the sentinel, the inputs hold their bits, and a second run gives the same bits (no
kernel of the family uses atomics).  A refused call leaves every output as it was.  Options are restored in `finally`.

kernel -> instantiation -> test [case ids]
  gemm_f32_kernel<0>, <1>       modes 0     test_f32_cross [*-tb0-*, *-tb1-*], test_f32_epilogues (act, accumulate, null bias, dwordx4 stores)
                                mode 1, 2   test_f32_two_products;  mode 3  test_f32_mirror;  mode 4  test_f32_heads [n0-n1]
                                stat_part   test_f32_stat_part;  refusals  test_f32_refusals
  gemm_sb_kernel<4>             K = 128     test_sb_rows [M-form4], test_sb_k [128-0], test_sb_natural_form [256-0-128, 128-1-128]
  gemm_sb_kernel<0>             other K     test_sb_k [32-0 .. 1152-0, 384-2], test_sb_k [128-0] under gsb_dbg bit 5, test_sb_natural_form [*-96]
    <NG, false, true> (FOUR)                the "bwd4" variant of the same tests;  <NG, true> (ONE)  test_sb_bf16_single [form4]
  gemm_sb16_kernel<4|8|12|16|24|36>         test_sb_k [128-0, 256-0, 384-0, 512-0, 384-2, 1152-0] (form 16), test_sb_rows [M-form16]
  gemm_sb16_kernel<0>                       test_sb_k [32-0, 96-0, 160-0] and every unrolled K again under gsb_dbg bit 4 (same bits)
    <NG, false, false, true> (FOUR)         the "bwd4" variant;  <4|24|0, false, true> (ONE)  test_sb_bf16_single [form16]
  gemm_sb16_kernel<0|36|72, true> (CONV)    test_sb_conv [C32-*, C128-*, C256-*];  <36, true, false, true>  test_sb_conv_dgrad
    epilogues (act, accum, null bias, mode 1, stat_part, addg + gate4) of both kernels: test_sb_epilogues, test_sb_stat_addg;  test_sb_refusals
  gemm_sbp_kernel                           test_kernels_gpu.py::test_gemm_k128_b_stationary_form_is_bit_identical (kept; M = 1 and 31 added)
  gemm_split_b_kernel           transb 0, 1, 2   every split-bf16 test above; test_weight_prep (planes add up to the weight, fused == alone)
  gemm_tn_kernel<32>, <64>                  test_tn [*-cr32-*, *-cr64-*] (splits, max_splits, leading dimensions, want_bias, shifts)
  gemm_tn_sb_kernel<false> six / four / one test_tn_sb_batch [M-N] (1, 2, 4 jobs), test_tn_sb_tiles [K1-N-M] (six, four)
  gemm_tn_sb_kernel<true> six / four        test_tn_sb_conv [C128-*, C256-*]
  reduce_slabs_kernel, reduce_slabs2_kernel test_reduce_slabs [nslab];  reduce_slabs_stage_kernel  test_reduce_two_stage [nslab]
  reduce_slabs2_batch_kernel                test_reduce_batch, test_tn_sb_batch
  heads_weff_kernel, heads_grad_kernel      test_heads [K-Hd-n0-n1], test_heads_refusals;  weight_prep_kernel  test_weight_prep [na-nb-weff]
  mul_kernel                                test_mul

The hand-made faults the file was tried against, and the tests that fail under each, are in DESIGN.md 3v."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import gemm_cases as G
import helpers
from gemm_cases import f64

pytestmark = pytest.mark.gpu

NAN = float("nan")
NAN_BITS = int(np.array(NAN, np.float32).view(np.int32))
BAND = 320           # floats in front of and behind a window: a multiple of 4 (an aligned base stays aligned) and more than any row written here, so a
                     # store one row past the last lands on sentinels, inside the allocation
DEFAULTS = {b"gsb_dbg": 0, b"bwd_four_products": 1, b"bf16_single": 0}


def _bits(t):
    return t.view(torch.int32)


class Win:
    """[rows, cols] floats at row stride ld, `front` floats into a NaN-filled allocation: the floats outside the window are sentinels"""

    def __init__(self, rows, cols, ld=None, data=None, off=0):
        ld = cols if ld is None else ld
        assert ld >= cols
        self.rows, self.cols, self.ld, front = rows, cols, ld, BAND + off
        self.buf = torch.full((front + rows * ld + BAND,), NAN, device="cuda")
        self.view = torch.as_strided(self.buf, (rows, cols), (ld, 1), front)
        self.outside = torch.ones(self.buf.numel(), dtype=torch.bool, device="cuda")
        torch.as_strided(self.outside, (rows, cols), (ld, 1), front).fill_(False)
        if data is not None:
            self.view.copy_(helpers.dev(np.array(data, np.float32).reshape(rows, cols)))      # a copy: the shared inputs are read-only
        self.saved = _bits(self.buf).clone()

    def ptr(self):
        return C.c_void_p(self.view.data_ptr())

    def unchanged(self):
        return torch.equal(_bits(self.buf), self.saved)

    def band_ok(self):
        return bool((_bits(self.buf)[self.outside] == NAN_BITS).all())

    def numpy(self):
        return self.view.contiguous().cpu().numpy()


def P(x):
    return None if x is None else x.ptr() if isinstance(x, Win) else C.c_void_p(x.data_ptr())


def settle(name, ins, outs):
    """after a call: inputs and their surroundings hold their bits, every float around an output window holds the sentinel"""
    torch.cuda.synchronize()
    for i, w in enumerate(ins):
        assert w is None or w.unchanged(), f"{name}: input {i}, or the band around it, was written"
    for i, w in enumerate(outs):
        assert w is None or w.band_ok(), f"{name}: a float outside output window {i} was written"


def untouched(name, outs):
    torch.cuda.synchronize()
    for i, w in enumerate(outs):
        assert w is None or w.unchanged(), f"{name}: a refused call wrote output {i}"


def same_bits(name, a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        if x is not None:
            assert torch.equal(_bits(x.buf), _bits(y.buf)), f"{name}: output {i} differs between two runs / two forms"


def twice(name, run):
    """run() makes fresh outputs, calls, and returns them: two runs give the same bits"""
    a, b = run(), run()
    same_bits(name + " (second run)", a, b)
    return a


@contextlib.contextmanager
def options(lib, **kw):
    try:
        for k, v in kw.items():
            assert lib.seld_k_set_option(k.encode(), v) == 0
        yield
    finally:
        for k, v in DEFAULTS.items():
            lib.seld_k_set_option(k, v)


def check_mag(name, got, ref, mag, bar=G.BAR6):
    helpers.check(name, got, ref)
    G.report(name + " / magnitude", G.mag_err(got, ref, mag), bar)


def ptrs(ws):
    return (C.c_void_p * len(ws))(*[w.view.data_ptr() if isinstance(w, Win) else w.data_ptr() for w in ws])


def ints(v):
    return (C.c_int * len(v))(*v)


# ================================================================ gemm_f32_kernel
def gemm_ex(lib, A, B, bias, Cw, M, N, K, transb=0, act=0, accumulate=0, mode=0, A1=None, B1=None, bias1=None, C1=None, M0=None, M1=None, nsplit=0,
            stat=None, addg=None):
    return lib.seld_k_gemm_ex(P(A), A.ld, P(B), B.ld, P(bias), P(Cw), Cw.ld, M, N, K, transb, act, accumulate, mode, P(A1), P(B1), P(bias1), P(C1),
                              P(M0), P(M1), nsplit, P(stat), P(addg))


@pytest.mark.parametrize("c", G.F32_CASES, ids=G.f32_id)
def test_f32_cross(seld_lib, c):
    A, B, bias, prev, A1, B1, bias1 = G.f32_inputs(c.M, c.N, c.K, c.transb)
    lda, ldb, ldc, off = G.f32_lds(c)
    wa, wb, wbias = Win(c.M, c.K, lda, A, off), Win(*B.shape, ldb, B, off), Win(1, c.N, data=bias)

    def run():
        wc = Win(c.M, c.N, ldc)
        assert gemm_ex(seld_lib, wa, wb, wbias, wc, c.M, c.N, c.K, c.transb) == 0
        settle(G.f32_id(c), (wa, wb, wbias), (wc,))
        return (wc,)
    (wc,) = twice(G.f32_id(c), run)
    check_mag("gemm_f32 " + G.f32_id(c), wc.numpy(), *G.product(A, B, c.transb, bias))


@pytest.mark.parametrize("shape", G.F32_EPI_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_f32_epilogues(seld_lib, shape):
    """act 0..3 x accumulate x bias / null bias, both transb; ldc % 4 == 0: whole 32 x 32 tiles leave through the dwordx4 stores, ragged ones do not"""
    M, N, K, ldc = shape
    for tb in (0, 1):
        A, B, bias, prev, A1, B1, bias1 = G.f32_inputs(M, N, K, tb)
        A = A * G.EPI_SCALE
        wa, wb, wbias = Win(M, K, data=A), Win(*B.shape, data=B), Win(1, N, data=bias)
        for act in range(4):
            for acc in (0, 1):
                for wbi, bi in ((wbias, bias), (None, None)):
                    name = f"gemm_f32 {M, N, K} tb{tb} act{act} acc{acc} bias{bi is not None}"

                    def run():
                        wc = Win(M, N, ldc, prev if acc else None)
                        assert gemm_ex(seld_lib, wa, wb, wbi, wc, M, N, K, tb, act, acc) == 0
                        settle(name, (wa, wb, wbias), (wc,))
                        return (wc,)
                    (wc,) = twice(name, run)
                    check_mag(name, wc.numpy(), *G.product(A, B, tb, bi, act, prev if acc else None))


def test_f32_two_products(seld_lib):
    """mode 1 (two products sharing A, different biases) and mode 2 (one product over a concatenated K, K = 32 and 64, with accumulate)"""
    M, N, K = 65, 130, 33
    for tb in (0, 1):
        A, B, bias, prev, A1, B1, bias1 = G.f32_inputs(M, N, K, tb)
        A = A * G.EPI_SCALE
        nat = K if tb else N
        wa, wb, wb1, wbi, wbi1 = Win(M, K, K + 1, A), Win(*B.shape, nat + 1, B), Win(*B.shape, nat + 1, B1), Win(1, N, data=bias), Win(1, N, data=bias1)

        def run():
            wc, wc1 = Win(M, N, N + 3), Win(M, N, N + 3)
            assert gemm_ex(seld_lib, wa, wb, wbi, wc, M, N, K, tb, 2, 0, 1, B1=wb1, bias1=wbi1, C1=wc1) == 0
            settle("mode 1", (wa, wb, wb1, wbi, wbi1), (wc, wc1))
            return wc, wc1
        wc, wc1 = twice("mode 1", run)
        check_mag(f"gemm_f32 mode 1 tb{tb} first", wc.numpy(), *G.product(A, B, tb, bias, 2))
        check_mag(f"gemm_f32 mode 1 tb{tb} second", wc1.numpy(), *G.product(A, B1, tb, bias1, 2))
    M, N = 65, 63
    for K in (32, 64):
        for tb in (0, 1):
            A, B, bias, prev, A1, B1, bias1 = G.f32_inputs(M, N, K, tb)
            nat = K if tb else N
            wa, wa1, wb, wb1, wbi = Win(M, K, K + 4, A), Win(M, K, K + 4, A1), Win(*B.shape, nat + 4, B), Win(*B.shape, nat + 4, B1), Win(1, N, data=bias)

            def run():
                wc = Win(M, N, N + 3, prev)
                assert gemm_ex(seld_lib, wa, wb, wbi, wc, M, N, K, tb, 0, 1, 2, A1=wa1, B1=wb1) == 0
                settle("mode 2", (wa, wa1, wb, wb1, wbi), (wc,))
                return (wc,)
            (wc,) = twice("mode 2", run)
            check_mag(f"gemm_f32 mode 2 K{K} tb{tb}", wc.numpy(), *G.product(A, B, tb, bias, 0, prev, A1, B1))


@pytest.mark.parametrize("shape", G.F32_EPI_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_f32_mirror(seld_lib, shape):
    """mode 3: the mirror holds the bits of C, through both store paths"""
    M, N, K, ldc = shape
    A, B, bias, prev, A1, B1, bias1 = G.f32_inputs(M, N, K, 0)
    A = A * G.EPI_SCALE
    wa, wb, wbi = Win(M, K, data=A), Win(K, N, data=B), Win(1, N, data=bias)
    wc, wm = Win(M, N, ldc), Win(M, N, ldc)
    assert gemm_ex(seld_lib, wa, wb, wbi, wc, M, N, K, 0, 1, 0, 3, C1=wm) == 0
    settle("mirror", (wa, wb, wbi), (wc, wm))
    check_mag(f"gemm_f32 mode 3 {M, N, K}", wc.numpy(), *G.product(A, B, 0, bias, 1))
    G.report_exact(f"gemm_f32 mode 3 {M, N, K} mirror == C", wm.numpy(), wc.numpy())


@pytest.mark.parametrize("n0,n1", G.F32_HEADS)
def test_f32_heads(seld_lib, n0, n1):
    """mode 4: both heads' outputs from one product; different activations, with and without the copies"""
    M, K, N = 65, 33, n0 + n1
    A, B, bias, prev, A1, B1, bias1 = G.f32_inputs(M, N, K, 0)
    A = A * G.EPI_SCALE
    wa, wb, wbi = Win(M, K, K + 1, A), Win(K, N, data=B), Win(1, N, data=bias)
    for act0, act1, copies in ((1, 2, True), (2, 1, False), (0, 1, True)):
        name = f"gemm_f32 mode 4 n{n0}+{n1} act{act0}{act1} copies{copies}"

        def run():
            outs = [Win(M, n0), Win(M, n1)] + ([Win(M, n0), Win(M, n1)] if copies else [None, None])
            # ldc plays no part: each head's rows are dense
            assert seld_lib.seld_k_gemm_ex(P(wa), wa.ld, P(wb), wb.ld, P(wbi), P(outs[0]), 0, M, N, K, 0, act0 | act1 << 4, 0, 4, None, None, None, P(outs[1]),
                                           P(outs[2]), P(outs[3]), n0, None, None) == 0
            settle(name, (wa, wb, wbi), outs)
            return outs
        outs = twice(name, run)
        r0, m0 = G.product(A, B[:, :n0], 0, bias[:n0], act0)
        r1, m1 = G.product(A, B[:, n0:], 0, bias[n0:], act1)
        check_mag(name + " C0", outs[0].numpy(), r0, m0)
        check_mag(name + " C1", outs[1].numpy(), r1, m1)
        if copies:
            G.report_exact(name + " M0 == C0", outs[2].numpy(), outs[0].numpy())
            G.report_exact(name + " M1 == C1", outs[3].numpy(), outs[1].numpy())


def test_f32_stat_part(seld_lib):
    M, N, K = G.F32_STAT
    for N_ in (N, 96):      # 96: the second column tile has 32 columns; the partial's other 32 are zeros
        A, B, bias, prev, A1, B1, bias1 = G.f32_inputs(M, N_, K, 0)
        wa, wb = Win(M, K, K + 1, A), Win(K, N_, data=B)

        def run():
            wc, wp = Win(M, N_, N_ + 3), Win(1, -(-N_ // 64) * -(-M // 64) * 128)
            assert gemm_ex(seld_lib, wa, wb, None, wc, M, N_, K, stat=wp) == 0
            settle("stat_part", (wa, wb), (wc, wp))
            return wc, wp
        wc, wp = twice("gemm_f32 stat_part", run)
        check_mag(f"gemm_f32 stat_part N{N_} product", wc.numpy(), *G.product(A, B))
        ref, mag = G.stat_ref(wc.numpy(), 64)
        check_mag(f"gemm_f32 stat_part N{N_} partials", wp.numpy(), ref, mag, G.BAR6)


def test_f32_refusals(seld_lib):
    for name, kw in G.F32_REFUSALS:
        M, N, K = max(kw["M"], 1), kw["N"], kw["K"]
        A, B, bias, prev, A1, B1, bias1 = G.f32_inputs(M, N, K, 0)
        wa, wa1, wb, wb1, wbi = Win(M, K, data=A), Win(M, K, data=A1), Win(K, N, data=B), Win(K, N, data=B1), Win(1, N, data=bias)
        wc, wp, wg = Win(M, N), Win(1, -(-N // 64) * -(-M // 64) * 128), Win(M, N, data=prev)
        mode = kw.get("mode", 0)
        rc = gemm_ex(seld_lib, wa, wb, wbi if kw.get("bias") or mode == 2 else None, wc, kw["M"], N, K, 0, kw.get("act", 0), kw.get("accumulate", 0), mode,
                     A1=wa1 if mode == 2 else None, B1=wb1 if mode == 2 else None, stat=wp if kw.get("stat") else None, addg=wg if kw.get("addg") else None)
        assert rc != 0, name
        untouched(name, (wc, wp))


# ================================================================ gemm_sb_kernel / gemm_sb16_kernel
def gemm_sb_ex(lib, A0, B0, bias0, C0, M, N, K, transb=0, act=0, mode=0, accum=0, backward=0, A1=None, B1=None, bias1=None, C1=None, stat=None, addg=None,
               gate4=None, conv=(0, 0, 0)):
    return lib.seld_k_gemm_sb_ex(P(A0), P(A1), A0.ld, P(B0), P(B1), B0.ld, transb, P(bias0), P(bias1), P(C0), P(C1), C0.ld, M, N, K, act, mode, accum, backward,
                                 P(stat), P(addg), P(gate4), *conv)


VARIANTS = {"fwd": (0, 0, 1, G.BAR6), "bwd4": (1, 1, 1, G.BAR4), "bwd6": (1, 1, 0, G.BAR6)}      # transb, backward, bwd_four_products, bar


def sb_run(lib, name, M, N, K, variant, dbg, mode=0, lda=None, ldc=None, act=0, accum=0, bias=True, ascale=None):
    """one product in one variant and one kernel form; returns the output windows after the checks against fp64"""
    tb, backward, four, bar = VARIANTS[variant]
    A0, A1, B0, B1, b0, b1, prev, addg = G.sb_inputs(M, N, K, tb)
    if ascale is not None:
        A0, A1 = A0 * ascale, A1 * ascale
    lda, ldc = lda or K, ldc or N
    wa0, wa1, wb0, wb1 = Win(M, K, lda, A0), Win(M, K, lda, A1), Win(*B0.shape, data=B0), Win(*B1.shape, data=B1)
    wbi0, wbi1 = (Win(1, N, data=b0), Win(1, N, data=b1)) if bias else (None, None)

    def run():
        wc, wc1 = Win(M, N, ldc, prev if accum else None), Win(M, N, ldc) if mode == 1 else None
        assert gemm_sb_ex(lib, wa0, wb0, wbi0, wc, M, N, K, tb, act, mode, accum, backward, A1=wa1 if mode == 2 else None, B1=wb1 if mode else None,
                          bias1=wbi1 if mode == 1 else None, C1=wc1) == 0, name
        settle(name, (wa0, wa1, wb0, wb1, wbi0, wbi1), (wc, wc1))
        return wc, wc1
    with options(lib, gsb_dbg=dbg, bwd_four_products=four):
        wc, wc1 = twice(name, run)
    kw = dict(A1=A1, B1=B1) if mode == 2 else {}
    check_mag(name, wc.numpy(), *G.product(A0, B0, tb, b0 if bias else None, act, prev if accum else None, **kw), bar)
    if mode == 1:
        check_mag(name + " second", wc1.numpy(), *G.product(A0, B1, tb, b1 if bias else None, act), bar)
    return wc, wc1


@pytest.mark.parametrize("form", (G.FORM4, G.FORM16), ids=("form4", "form16"))
@pytest.mark.parametrize("M", G.SB_MS)
def test_sb_rows(seld_lib, M, form):
    """every row count in either kernel form (gsb_dbg bits 2, 3), forward and the four-product backward; lda = K + 4, ldc = N + 4"""
    for v in ("fwd", "bwd4"):
        sb_run(seld_lib, f"gemm_sb M{M} form{form} {v}", M, 128, 128, v, form, lda=132, ldc=132)


@pytest.mark.parametrize("K,mode", G.SB_KS)
def test_sb_k(seld_lib, K, mode):
    """every unrolled instance and the runtime loops, in every variant; the generic loops (gsb_dbg bits 4, 5) give the bits of the unrolled ones.
    ldc = N + 1: no dwordx4 stores"""
    M, N = 129, 128
    for form in (G.FORM4, G.FORM16):
        generic = G.GENERIC16 if form == G.FORM16 and (K, mode) in G.SB_UNROLLED16 else G.GENERIC4 if form == G.FORM4 and K == 128 and mode != 2 else 0
        for v in G.SB_VARIANTS:
            name = f"gemm_sb K{K} mode{mode} form{form} {v}"
            outs = sb_run(seld_lib, name, M, N, K, v, form, mode, ldc=N + 1)
            if generic:
                same_bits(name + ": generic loop == unrolled", outs, sb_run(seld_lib, name + " generic", M, N, K, v, form | generic, mode, ldc=N + 1))


@pytest.mark.parametrize("N,mode,K", G.SB_NATURAL)
def test_sb_natural_form(seld_lib, N, mode, K):
    """what the launcher picks by itself: two column groups (N = 256, or mode 1 at N = 128) take the 4-wave kernel; N = 128 the 16-wave kernel,
    whose bits equal the forced form's"""
    for v in ("fwd", "bwd4"):
        sb_run(seld_lib, f"gemm_sb N{N} mode{mode} K{K} {v}", 129, N, K, v, 0, mode, ldc=N + 4)
    if mode == 0:
        same_bits("natural == forced 16-wave form", sb_run(seld_lib, "gemm_sb N128 natural", 129, 128, K, "fwd", 0),
                  sb_run(seld_lib, "gemm_sb N128 form16", 129, 128, K, "fwd", G.FORM16))


@pytest.mark.parametrize("form", (G.FORM4, G.FORM16), ids=("form4", "form16"))
def test_sb_epilogues(seld_lib, form):
    """act x accum x bias / null bias through the guarded stores (and the 16-wave kernel's dwordx4 path: ldc % 4 == 0), mode 1 with two biases.
    The four-product form runs without an activation, as every backward product of the model does: its error is a fraction of |A| |B|, which on
    these inputs is hundreds of times a sigmoid's or tanh's range (measured: 6.6e-4 of the tensor at act 1), so an activation behind it is no case
    of this form; accum and the null bias reach its guarded stores all the same."""
    M, N, K = 129, 128, 96
    for act in range(4):
        for accum in (0, 1):
            for bias in (True, False):
                for v in ("fwd", "bwd4") if act == 0 else ("fwd",):
                    sb_run(seld_lib, f"gemm_sb form{form} act{act} accum{accum} bias{bias} {v}", M, N, K, v, form, act=act, accum=accum, bias=bias, lda=K + 4, ldc=N + 4, ascale=G.EPI_SCALE)
    sb_run(seld_lib, f"gemm_sb form{form} mode 1 act 2", M, N, K, "fwd", form, mode=1, act=2, ldc=N + 1, ascale=G.EPI_SCALE)
    sb_run(seld_lib, f"gemm_sb form{form} mode 1 K128", M, N, 128, "bwd4", form, mode=1, ldc=N + 4)


@pytest.mark.parametrize("form", (G.FORM4, G.FORM16), ids=("form4", "form16"))
@pytest.mark.parametrize("M", (129, 33))
def test_sb_stat_addg(seld_lib, M, form):
    """the GemmEpi epilogues: BatchNorm partials per (128-row block, column), and C += addg where the gate bit of element row * ldc + col is set"""
    N, K, ldc = 128, 128, 132
    with options(seld_lib, gsb_dbg=form):
        A0, A1, B0, B1, b0, b1, prev, addg = G.sb_inputs(M, N, K, 0)
        wa, wb = Win(M, K, K + 4, A0), Win(K, N, data=B0)

        def run_stat():
            wc, wp = Win(M, N, ldc), Win(1, N // 64 * -(-M // 128) * 128)
            assert gemm_sb_ex(seld_lib, wa, wb, None, wc, M, N, K, stat=wp) == 0
            settle("stat_part", (wa, wb), (wc, wp))
            return wc, wp
        wc, wp = twice("gemm_sb stat_part", run_stat)
        check_mag(f"gemm_sb stat_part M{M} form{form} product", wc.numpy(), *G.product(A0, B0))
        check_mag(f"gemm_sb stat_part M{M} form{form} partials", wp.numpy(), *G.stat_ref(wc.numpy(), 128), G.BAR6)
        # the gated add, as the model takes it: a backward product, accumulate on and off
        A0, A1, B0, B1, b0, b1, prev, addg = G.sb_inputs(M, N, K, 1)
        wa, wb, wg = Win(M, K, K + 4, A0), Win(N, K, data=B0), Win(M, N, ldc, addg)
        for all_off in (False, True):
            for accum in (0, 1):
                g, on = G.gates(M, ldc, all_off=all_off)
                gd = torch.as_tensor(np.array(g)).cuda()
                name = f"gemm_sb addg M{M} form{form} off{all_off} accum{accum}"

                def run_addg(gate=gd, add=wg):
                    wc = Win(M, N, ldc, prev if accum else None)
                    assert gemm_sb_ex(seld_lib, wa, wb, None, wc, M, N, K, 1, 0, 0, accum, 1, addg=add, gate4=gate) == 0
                    settle(name, (wa, wb, wg), (wc,))
                    assert torch.equal(gd.cpu(), torch.as_tensor(np.array(g)))
                    return (wc,)
                (wc,) = twice(name, run_addg)
                ref, mag = G.product(A0, B0, 1, None, 0, prev if accum else None)
                check_mag(name, wc.numpy(), ref + on[:, :N] * f64(addg), mag + on[:, :N] * np.abs(f64(addg)), G.BAR4)
                if all_off:      # zero by construction: the bits of the same product without the epilogue
                    same_bits(name + " == no addg", (wc,), run_addg(None, None))


@pytest.mark.parametrize("C_,img", G.SB_CONV, ids=lambda v: str(v).replace(" ", ""))
def test_sb_conv(seld_lib, C_, img):
    """implicit 3 x 3 'same' convolution against fp64 conv2d: every pixel on a border, batch boundaries inside the tile"""
    x, w, dz = G.conv_inputs(C_, img)
    M, N, K = int(np.prod(img)), w.shape[3], 9 * C_
    wx, ww, wbi = Win(M, C_, data=x), Win(K, N, data=w), Win(1, N, data=G.f32_inputs(1, N, 1, 0)[2])

    def run():
        wc = Win(M, N, N + 4)
        assert gemm_sb_ex(seld_lib, wx, ww, wbi, wc, M, N, K, conv=(C_, img[1], img[2])) == 0
        settle("conv", (wx, ww, wbi), (wc,))
        return (wc,)
    (wc,) = twice("conv", run)
    ref, mag = G.conv_fwd_ref(x, w)
    bias = f64(G.f32_inputs(1, N, 1, 0)[2])
    check_mag(f"gemm_sb16 conv C{C_} {img}", wc.numpy(), ref + bias, mag + np.abs(bias))


@pytest.mark.parametrize("C_,img", G.SB_CONV_BWD, ids=lambda v: str(v).replace(" ", ""))
def test_sb_conv_dgrad(seld_lib, C_, img):
    """the input gradient of the same convolution: the kernel read as the flipped, channel-swapped matrix (transb 2), four products and six"""
    x, w, dz = G.conv_inputs(C_, img)
    M, N = int(np.prod(img)), w.shape[3]
    wdz, ww = Win(M, N, data=dz), Win(9 * C_, N, data=w)
    dx, _ = G.conv_grads_ref(x, w, dz)
    mag = np.abs(f64(G.im2col3x3(dz))) @ np.abs(f64(G.dgrad_matrix(w)))
    for four, bar in ((1, G.BAR4), (0, G.BAR6)):
        def run():
            wc = Win(M, C_, C_ + 4)
            assert gemm_sb_ex(seld_lib, wdz, ww, None, wc, M, C_, 9 * N, 2, backward=1, conv=(N, img[1], img[2])) == 0
            settle("conv dgrad", (wdz, ww), (wc,))
            return (wc,)
        with options(seld_lib, bwd_four_products=four):
            (wc,) = twice("conv dgrad", run)
        check_mag(f"gemm_sb16 conv dgrad C{C_} {img} four{four}", wc.numpy(), dx, mag, bar)


def test_sb_refusals(seld_lib):
    for name, kw in G.SB_REFUSALS:
        M, N, K = kw["M"], kw["N"], kw["K"]
        ldc, mode = kw.get("ldc", N), kw.get("mode", 0)
        rng = np.random.default_rng(1)
        wa0, wa1 = Win(M, K, data=G.binade(rng, (M, K))), Win(M, K, data=G.binade(rng, (M, K)), off=kw.get("a1_off", 0))
        wb, wbi = Win(K, N, data=G.binade(rng, (K, N))), Win(1, N, data=G.binade(rng, (N,)))
        wc, wp, wg = Win(M, N, ldc), Win(1, -(-N // 64) * -(-M // 128) * 128), Win(M, N, ldc, G.binade(rng, (M, N)))
        gd = torch.as_tensor(np.array(G.gates(M, ldc)[0])).cuda()
        rc = gemm_sb_ex(seld_lib, wa0, wb, wbi if kw.get("bias") else None, wc, M, N, K, 0, 0, mode, A1=wa1 if mode == 2 else None, B1=wb if mode else None,
                        stat=wp if kw.get("stat") else None, addg=wg if kw.get("addg") else None, gate4=gd if kw.get("addg") and kw.get("gate", True) else None,
                        conv=(kw.get("conv_C", 0), kw.get("H", 0), kw.get("W", 0)))
        assert rc != 0, name
        untouched(name, (wc, wp))
    # a backward product wants the planes of a transposed job
    wa, wb, wc = Win(33, 96), Win(96, 128), Win(33, 128)
    assert gemm_sb_ex(seld_lib, wa, wb, None, wc, 33, 128, 96, 0, backward=1) != 0
    untouched("backward with transb 0", (wc,))


@pytest.mark.parametrize("form", (G.FORM4, G.FORM16), ids=("form4", "form16"))
def test_sb_bf16_single(seld_lib, form):
    """bf16 single-product mode: the kernel agrees with the fp64 product of the bf16-rounded operands to 2e-6 (test_bf16_single_product_conv64):
    K = 128 and K = 2 x 384 in mode 2 (the unrolled single-product instances of the 16-wave kernel) and K = 96 (the generic loop)"""
    M, N = 129, 128
    for K, mode in ((128, 0), (384, 2), (96, 0)):
        A0, A1, B0, B1, b0, b1, prev, addg = G.sb_inputs(M, N, K, 0)
        wa0, wa1, wb0, wb1, wbi = Win(M, K, K + 4, A0), Win(M, K, K + 4, A1), Win(K, N, data=B0), Win(K, N, data=B1), Win(1, N, data=b0)

        def run():
            wc = Win(M, N, N + 4)
            assert gemm_sb_ex(seld_lib, wa0, wb0, wbi, wc, M, N, K, 0, 0, mode, A1=wa1 if mode else None, B1=wb1 if mode else None) == 0
            settle("bf16_single", (wa0, wa1, wb0, wb1, wbi), (wc,))
            return (wc,)
        with options(seld_lib, gsb_dbg=form, bf16_single=1):
            (wc,) = twice("bf16_single", run)
        ref = G.bf16_rne(A0) @ G.bf16_rne(B0) + f64(b0) + (G.bf16_rne(A1) @ G.bf16_rne(B1) if mode else 0.0)
        helpers.check(f"gemm_sb bf16_single K{K} mode{mode} form{form} vs fp64 of rounded operands", wc.numpy(), ref, tol=G.BAR1)
        exact, _ = G.product(A0, B0, 0, b0, **(dict(A1=A1, B1=B1) if mode else {}))
        print(f"[bf16] K{K} mode{mode} form{form}: error of the mode against the unrounded fp64 result {helpers.rel_err(wc.numpy(), exact):.2e}")


# ================================================================ gemm_tn_kernel
@pytest.mark.parametrize("c", G.TN_CASES, ids=G.tn_id)
def test_tn(seld_lib, c):
    """fp32 A^T B over row splits, then reduce_slabs / reduce_slabs2: the product's bits do not depend on want_bias; a shift takes A's rows from the
    neighbour inside each sequence, and with S = 1 the result is exactly zero"""
    name = "gemm_tn " + G.tn_id(c)
    A, B = G.tn_inputs(c.M, c.K1, c.N)
    pad, off = (c.pad, 0) if c.pad >= 0 else (0, 1)
    wa, wb = Win(c.M, c.K1, c.K1 + pad, A, off), Win(c.M, c.N, c.N + pad, B, off)

    def run(bias=1):
        wc, wcs = Win(c.K1, c.N), Win(1, c.N) if bias else None
        ns = C.c_int(-1)
        assert seld_lib.seld_k_gemm_tn_ex(P(wa), wa.ld, P(wb), wb.ld, P(wc), P(wcs), c.M, c.K1, c.N, c.S, c.shift, bias, c.max_splits, c.chunk, C.byref(ns)) == 0
        assert ns.value == c.nslab
        settle(name, (wa, wb), (wc, wcs))
        return wc, wcs
    wc, wcs = twice(name, run)
    ref, mag, cs, csmag = G.tn_ref(A, B, c.M, c.S, c.shift)
    check_mag(name, wc.numpy(), ref, mag)
    check_mag(name + " colsum", wcs.numpy(), cs.reshape(1, -1), csmag.reshape(1, -1))
    same_bits(name + ": want_bias off", (wc,), run(0)[:1])
    if c.S == 1:
        assert not wc.numpy().any()


# ================================================================ gemm_tn_sb_kernel
TNSB_BARS = {"six": (dict(bwd_four_products=0), G.BAR6), "four": (dict(bwd_four_products=1), G.BAR4), "one": (dict(bf16_single=1), None)}


def tnsb_check(name, form, got, A, B, M, S, shift):
    ref, mag, cs, csmag = G.tn_ref(A, B, M, S, shift)
    if form == "one":
        helpers.check(name + " vs fp64 of rounded operands", got, G.bf16_rne(G.shifted(A, M, S if S else M, shift)).T @ G.bf16_rne(B), tol=G.BAR1)
    else:
        check_mag(name, got, ref, mag, TNSB_BARS[form][1])
    return cs.reshape(1, -1), csmag.reshape(1, -1)


@pytest.mark.parametrize("N", (128, 256))
@pytest.mark.parametrize("M", G.TNSB_MS)
def test_tn_sb_batch(seld_lib, M, N):
    """1, 2 and 4 jobs whose A, lda and shift differ: each against its own fp64 product, each equal to the single-job launch bit for bit"""
    S = G.TNSB_S
    ins = [G.tnsb_inputs(M, N, j) for j in range(G.TN_MAX_JOBS)]
    was = [Win(A.shape[0], 128, 128 + dl, A) for (A, B), (sh, dl) in zip(ins, G.TNSB_JOBS)]
    wbs = [Win(M, N, N + 4, B) for A, B in ins]
    for form in G.TNSB_FORMS:
        def run(jobs):
            wcs, wss = [Win(128, N) for _ in jobs], [Win(1, N) for _ in jobs]
            ns = C.c_int(-1)
            rc = seld_lib.seld_k_gemm_tn_sb_ex(len(jobs), ptrs([was[j] for j in jobs]), ints([was[j].ld for j in jobs]), ints([G.TNSB_JOBS[j][0] for j in jobs]),
                                               ptrs([wbs[j] for j in jobs]), N + 4, ptrs(wcs), ptrs(wss), M, N, S, 1, C.byref(ns))
            assert rc == 0 and ns.value == G.tn_splits(M)
            settle(f"tn_sb {form} {jobs}", was + wbs, wcs + wss)
            return wcs + wss
        with options(seld_lib, **TNSB_BARS[form][0]):
            full = twice(f"tn_sb {form}", lambda: run((0, 1, 2, 3)))
            for j in range(4):
                name = f"gemm_tn_sb M{M} N{N} {form} job{j}"
                cs, csmag = tnsb_check(name, form, full[j].numpy(), *ins[j], M, S, G.TNSB_JOBS[j][0])
                check_mag(name + " colsum", full[4 + j].numpy(), cs, csmag)
                single = run((j,))
                same_bits(name + ": batch of 4 == single launch", (full[j], full[4 + j]), single)
                if j == 2:
                    pair = run((2, 1))
                    same_bits(name + ": batch of 2 == single launch", (pair[0], pair[2]), single)
                    same_bits(name + ": batch of 2, second job", (pair[1], pair[3]), (full[1], full[5]))


def tn_tiles(lib, wa, wb, M, K1, N, cap, conv=(0, 0, 0)):
    wc, ns = Win(K1, N), C.c_int(-1)
    assert lib.seld_k_gemm_tn_sb_tiles(P(wa), wa.ld, P(wb), wb.ld, P(wc), M, K1, N, cap, *conv, C.byref(ns)) == 0
    settle("tn_sb tiles", (wa, wb), (wc,))
    return wc, ns.value


@pytest.mark.parametrize("K1,N,M", G.TNSB_TILES)
def test_tn_sb_tiles(seld_lib, K1, N, M):
    """tile mode: slab space for exactly one split, and for as many as the rows allow"""
    A, B = G.tn_inputs(M, K1, N)
    wa, wb = Win(M, K1, K1 + 4, A), Win(M, N, N + 4, B)
    ref, mag, _, _ = G.tn_ref(A, B, M)
    for form in G.TN_TILE_FORMS:
        with options(seld_lib, **TNSB_BARS[form][0]):
            for cap, want in ((K1 * N, 1), (8 * K1 * N, (M + 127) // 128)):
                got = []

                def run():
                    wc, ns = tn_tiles(seld_lib, wa, wb, M, K1, N, cap)
                    got.append(ns)
                    return (wc,)
                (wc,) = twice("tiles", run)
                assert got == [want, want] == [G.tn_tile_splits(M, K1, N, cap)] * 2
                check_mag(f"gemm_tn_sb tiles K{K1} N{N} M{M} {form} splits{want}", wc.numpy(), ref, mag, TNSB_BARS[form][1])
    wc = Win(K1, N)
    assert seld_lib.seld_k_gemm_tn_sb_tiles(P(wa), wa.ld, P(wb), wb.ld, P(wc), M, K1, N, K1 * N - 1, 0, 0, 0, C.byref(C.c_int())) != 0      # no room for one slab
    untouched("tiles without slab space", (wc,))


@pytest.mark.parametrize("C_,img", G.TNSB_CONV, ids=lambda v: str(v).replace(" ", ""))
def test_tn_sb_conv(seld_lib, C_, img):
    """the kernel gradient of the 3 x 3 convolution (implicit im2col rows) against the fp64 gradient of conv2d"""
    x, w, dz = G.conv_inputs(C_, img)
    M, N = int(np.prod(img)), w.shape[3]
    wx, wdz = Win(M, C_, data=x), Win(M, N, N + 4, dz)
    _, dw = G.conv_grads_ref(x, w, dz)
    mag = np.abs(f64(G.im2col3x3(x))).T @ np.abs(f64(dz.reshape(M, N)))
    for form in G.TN_TILE_FORMS:
        with options(seld_lib, **TNSB_BARS[form][0]):
            (wc,) = twice("tn conv", lambda: tn_tiles(seld_lib, wx, wdz, M, 9 * C_, N, 4 * 9 * C_ * N, (C_, img[1], img[2]))[:1])
        check_mag(f"gemm_tn_sb conv C{C_} {img} {form}", wc.numpy(), dw, mag, TNSB_BARS[form][1])


# ================================================================ reductions
@pytest.mark.parametrize("nslab", G.RED_NSLABS)
def test_reduce_slabs(seld_lib, nslab):
    """out (+)= the fp64 sum of the slabs, for every remainder of the 8-way grouping and the 4-in-flight loop; stride > n; then slabs2 with the
    boundary between its two outputs inside a 32-output block"""
    for n in G.RED_NS:
        stride = n + 3
        s = G.slabs(nslab, stride)
        ws = Win(nslab, n, stride, s[:, :n])
        prev = G.slabs(1, n, seed=4)
        for acc in (0, 1):
            name = f"reduce_slabs nslab{nslab} n{n} acc{acc}"

            def run():
                wo = Win(1, n, data=prev if acc else None)
                assert seld_lib.seld_k_reduce_slabs_ex(0, P(ws), nslab, stride, P(wo), n, None, 0, acc, None) == 0
                settle(name, (ws,), (wo,))
                return (wo,)
            (wo,) = twice(name, run)
            ref, mag = f64(s[:, :n]).sum(0, keepdims=True), np.abs(f64(s[:, :n])).sum(0, keepdims=True)
            check_mag(name, wo.numpy(), ref + (f64(prev) if acc else 0), mag + (np.abs(f64(prev)) if acc else 0))
    n_w, n_b, stride = 30, 5, 37
    s = G.slabs(nslab, stride)
    ws = Win(nslab, n_w + n_b, stride, s[:, :35])

    def run2():
        ww, wb = Win(1, n_w), Win(1, n_b)
        assert seld_lib.seld_k_reduce_slabs_ex(1, P(ws), nslab, stride, P(ww), n_w, P(wb), n_b, 0, None) == 0
        settle("slabs2", (ws,), (ww, wb))
        return ww, wb
    ww, wb = twice("slabs2", run2)
    tot, mag = f64(s[:, :35]).sum(0, keepdims=True), np.abs(f64(s[:, :35])).sum(0, keepdims=True)
    check_mag(f"reduce_slabs2 nslab{nslab} main", ww.numpy(), tot[:, :30], mag[:, :30])
    check_mag(f"reduce_slabs2 nslab{nslab} tail", wb.numpy(), tot[:, 30:], mag[:, 30:])


@pytest.mark.parametrize("nslab", G.RED_2STAGE)
def test_reduce_two_stage(seld_lib, nslab):
    n, stride = 100, 104
    groups = seld_lib.seld_k_reduce_slabs_groups(nslab)
    assert groups == (nslab + 63) // 64
    s = G.slabs(nslab, stride)
    ws = Win(nslab, n, stride, s[:, :n])

    def run():
        wo, wt = Win(1, n), Win(groups, n)
        assert seld_lib.seld_k_reduce_slabs_ex(2, P(ws), nslab, stride, P(wo), n, None, 0, 0, P(wt)) == 0
        settle("two-stage", (ws,), (wo, wt))
        return wo, wt
    wo, wt = twice("two-stage", run)
    check_mag(f"reduce_slabs two-stage nslab{nslab}", wo.numpy(), f64(s[:, :n]).sum(0, keepdims=True), np.abs(f64(s[:, :n])).sum(0, keepdims=True))
    tref = np.stack([f64(s[g * 64:(g + 1) * 64, :n]).sum(0) for g in range(groups)])
    tmag = np.stack([np.abs(f64(s[g * 64:(g + 1) * 64, :n])).sum(0) for g in range(groups)])
    check_mag(f"reduce_slabs two-stage nslab{nslab} groups", wt.numpy(), tref, tmag)


def test_reduce_batch(seld_lib):
    """three jobs' slabs one after another, each to its own pair of outputs"""
    nslab, n_w, n_b, stride = 9, 30, 5, 37
    s = G.slabs(3 * nslab, stride)
    ws = Win(3 * nslab, 35, stride, s[:, :35])

    def run():
        ww, wb = [Win(1, n_w) for _ in range(3)], [Win(1, n_b) for _ in range(3)]
        assert seld_lib.seld_k_reduce_slabs2_batch(P(ws), nslab, stride, 3, ptrs(ww), ptrs(wb), n_w, n_b) == 0
        settle("batch", (ws,), ww + wb)
        return ww + wb
    outs = twice("reduce batch", run)
    for j in range(3):
        blk = f64(s[j * nslab:(j + 1) * nslab, :35])
        tot, mag = blk.sum(0, keepdims=True), np.abs(blk).sum(0, keepdims=True)
        check_mag(f"reduce_slabs2_batch job{j} main", outs[j].numpy(), tot[:, :30], mag[:, :30])
        check_mag(f"reduce_slabs2_batch job{j} tail", outs[3 + j].numpy(), tot[:, 30:], mag[:, 30:])


# ================================================================ heads, weight_prep, mul
def heads_windows(heads):
    return [[Win(1, a.size, data=a) for a in h] for h in heads]


@pytest.mark.parametrize("K,Hd,n0,n1", G.HEADS_CASES)
def test_heads(seld_lib, K, Hd, n0, n1):
    """the folded head weights and the heads' gradients against the fp64 formulas above heads_weff_kernel"""
    heads, F, cs = G.heads_inputs(K, Hd, n0, n1)
    hw = heads_windows(heads)
    col = lambda i: ptrs([hw[0][i], hw[1][i]])
    flat = [w for h in hw for w in h]
    n, NT = ints((n0, n1)), n0 + n1

    def run():
        we = Win(K + 1, NT)
        assert seld_lib.seld_k_heads_weff(col(0), col(1), col(2), col(3), n, K, Hd, P(we)) == 0
        settle("weff", flat, (we,))
        return (we,)
    (we,) = twice("weff", run)
    check_mag(f"heads_weff {K, Hd, n0, n1}", we.numpy(), *G.heads_weff_ref(heads))
    wF, wcs = Win(K, NT, data=F), Win(1, NT, data=cs)

    def run_grad():
        outs = [[Win(K, Hd), Win(1, Hd), Win(Hd, nn), Win(1, nn)] for nn in (n0, n1)]
        o = lambda i: ptrs([outs[0][i], outs[1][i]])
        assert seld_lib.seld_k_heads_grad(col(0), col(1), col(2), o(0), o(1), o(2), o(3), n, K, Hd, P(wF), P(wcs)) == 0
        settle("heads_grad", flat + [wF, wcs], outs[0] + outs[1])
        return outs[0] + outs[1]
    outs = twice("heads_grad", run_grad)
    for hd, grads in enumerate(G.heads_grad_ref(heads, F, cs)):
        for i, (label, (ref, mag)) in enumerate(zip(("dW1", "db1", "dW2", "db2"), grads)):
            got = outs[4 * hd + i].numpy()
            check_mag(f"heads_grad {K, Hd, n0, n1} head{hd} {label}", got, ref.reshape(got.shape), mag.reshape(got.shape))


def test_heads_refusals(seld_lib):
    heads, F, cs = G.heads_inputs(5, 3, 30, 35)
    hw = heads_windows(heads)
    col = lambda i: ptrs([hw[0][i], hw[1][i]])
    we = Win(6, 65)
    assert G.heads_refuses(5, 30, 35)
    assert seld_lib.seld_k_heads_weff(col(0), col(1), col(2), col(3), ints((30, 35)), 5, 3, P(we)) != 0
    untouched("n0 + n1 = 65", (we,))
    # launch_weight_prep: K + 1 rows of Weff beyond its 4 x 144 block rows
    heads, F, cs = G.heads_inputs(576, 2, 1, 2)
    hw = heads_windows(heads)
    we, we2 = Win(577, 3), Win(577, 3)
    assert G.heads_refuses(576, 1, 2, prep=True)
    rc = seld_lib.seld_k_weight_prep(0, None, None, None, None, None, None, None, 0, None, None, None, None, col(0), col(1), col(2), col(3), ints((1, 2)), 576, 2,
                                     P(we), P(we2))
    assert rc != 0
    untouched("K + 1 > 576", (we, we2))


def planes(n_shorts):
    return torch.full((n_shorts + 64,), -1, dtype=torch.int16, device="cuda")


@pytest.mark.parametrize("na,nb,weff", G.PREP_CASES)
def test_weight_prep(seld_lib, na, nb, weff):
    """the merged pre-pass launch writes the bits of the three stand-alone kernels; the planes of a forward job add up to the weight exactly"""
    rng = np.random.default_rng([na, nb])
    shapes = [G.PREP_SHAPES[i % 4] for i in range(na)]
    srcs = [Win(*((N, K) if tb else (K, N)), data=G.binade(rng, (N, K) if tb else (K, N))) for K, N, tb in shapes]
    a_f, a_a = [planes(3 * K * N) for K, N, tb in shapes], [planes(3 * K * N) for K, N, tb in shapes]
    cw = [Win(9 * 64, 64, data=G.binade(rng, (9 * 64, 64))) for _ in range(nb)]
    b_f, b_a = [planes(9 * 3 * 4096) for _ in range(nb)], [planes(9 * 3 * 4096) for _ in range(nb)]
    K, Hd, n0, n1 = 128, 128, 14, 50
    heads, F, cs = G.heads_inputs(K, Hd, n0, n1)
    hw = heads_windows(heads)
    col = lambda i: ptrs([hw[0][i], hw[1][i]])
    we_f, we_a = (Win(K + 1, n0 + n1), Win(K + 1, n0 + n1)) if weff else (None, None)
    rc = seld_lib.seld_k_weight_prep(na, ptrs(srcs) if na else None, ints([s.ld for s in srcs]), ints([s[2] for s in shapes]), ints([s[0] for s in shapes]),
                                     ints([s[1] for s in shapes]), ptrs(a_f) if na else None, ptrs(a_a) if na else None, nb, ptrs(cw) if nb else None,
                                     ints([i % 2 for i in range(nb)]), ptrs(b_f) if nb else None, ptrs(b_a) if nb else None, col(0), col(1), col(2), col(3),
                                     ints((n0, n1)), K, Hd, P(we_f), P(we_a))
    assert rc == 0
    settle("weight_prep", srcs + cw + [w for h in hw for w in h], [w for w in (we_f, we_a) if w is not None])
    for label, fused, alone, sizes in (("gemm split", a_f, a_a, [3 * K_ * N_ for K_, N_, _ in shapes]), ("conv split", b_f, b_a, [9 * 3 * 4096] * nb)):
        for i, (f, a, size) in enumerate(zip(fused, alone, sizes)):
            G.report_exact(f"weight_prep {na, nb, weff} {label} job{i}: fused == stand-alone", f.cpu().numpy(), a.cpu().numpy())
            assert bool((f[size:] == -1).all()) and bool((f[:size].view(torch.int16) != -1).any())
    if weff:
        G.report_exact(f"weight_prep {na, nb, weff} weff: fused == stand-alone", we_f.numpy(), we_a.numpy())
        check_mag(f"weight_prep {na, nb, weff} weff", we_f.numpy(), *G.heads_weff_ref(heads))
    if na:      # job 0 ([K][N], transb 0): planes [k / 32][plane][n][piece ^ ((n >> 2) & 3)][8] of truncated bf16 add up to the weight
        K_, N_, _ = shapes[0]
        pl = a_f[0][:3 * K_ * N_].cpu().numpy().view(np.uint16).astype(np.uint32).reshape(K_ // 32, 3, N_, 4, 8)
        k, nn = np.meshgrid(np.arange(K_), np.arange(N_), indexing="ij")
        v = pl[k >> 5, :, nn, ((k & 31) >> 3) ^ ((nn >> 2) & 3), k & 7]                   # [K, N, 3]
        vals = (v << 16).astype(np.uint32).view(np.float32).astype(np.float64)
        G.report_exact("gemm_split_b planes: hi + mid + lo == w", vals.sum(-1), f64(srcs[0].numpy()))
        G.report_exact("gemm_split_b planes: hi == the upper 16 bits", v[..., 0], srcs[0].numpy().view(np.uint32) >> 16)


def test_weight_prep_nothing_to_do(seld_lib):
    assert seld_lib.seld_k_weight_prep(0, None, None, None, None, None, None, None, 0, None, None, None, None, None, None, None, None, None, 0, 0, None, None) == 0


def test_mul(seld_lib):
    for n in G.MUL_NS:
        a, b = (G.binade(np.random.default_rng([n, i]), (n,)) for i in range(2))
        wa, wb = Win(1, n, data=a), Win(1, n, data=b)

        def run():
            wo = Win(1, n)
            assert seld_lib.seld_k_mul(P(wa), P(wb), P(wo), n) == 0
            settle("mul", (wa, wb), (wo,))
            return (wo,)
        (wo,) = twice("mul", run)
        G.report_exact(f"mul n{n}", wo.numpy().reshape(-1), (f64(a) * f64(b)).astype(np.float32))
    wa, wo = Win(1, 8, data=np.ones(8)), Win(1, 8)
    assert seld_lib.seld_k_mul(P(wa), P(wa), P(wo), 6) != 0
    untouched("mul n = 6", (wo,))
