"""Every seld_m_* module operator (module_ops.hip; modules.py composes mother_block / mother_stage from them) on its own, against a float64
restatement of the same operation, at the edges where such kernels go wrong and at the shapes bench.py's mother_stage leg runs.

Each call goes to a non-default stream, which is synchronised before the result is read; outputs are prefilled with NaN, or with random
values for the accumulating forms.  Inputs carry a per-channel offset (mean 3 + c / C) so a channel mix-up or a wrong mean cannot hide
near zero.  Two bars: the project's tensor-normalised 1e-4 (helpers.check) everywhere, and the tighter one each operator's arithmetic
promises (double sums: one fp32 rounding of fp64; copies: bit for bit; ...).  The BatchNormalization case table is checked against a
restatement of the kernels' dispatch rule so that every path and every branch of the partial-sum fold stays covered."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import check, dev, ptr

pytestmark = pytest.mark.gpu

# ---- bench.py's mother_stage leg, restated (tests/test_module_ops_cpu.py checks it against bench.MOTHER_STAGE_ARGS)
BENCH_B, BENCH_T = 32, 3000
MOTHER_STAGE_ARGS = {"depth": 2, "filters0": 0, "filters1": 96, "filters2": 0, "kernel_size0": 0, "kernel_size1": 3, "kernel_size2": 0,
                     "connect0": [1], "connect1": [1, 0], "connect2": [1, 0, 1], "strides": [5, 3]}


def bench_shapes():
    """(in, out) (H, W, C) of each block of the stage and the GRU's input width, through oracle.modules_oracle.mother_block_plan"""
    from oracle import modules_oracle as M
    shape, blocks = (BENCH_T, 64, 7), []
    for d, cfg in enumerate(M.stage_configs(MOTHER_STAGE_ARGS)):
        out = M.mother_block_plan(cfg, shape, f"mb{d}")[2]
        blocks.append((shape, out))
        shape = out
    return {"blocks": blocks, "gru_in": shape[1] * shape[2]}


# ---- the BatchNormalization sums' dispatch (module_ops.hip: bnp_blocks, seld_m_bn_stats / seld_m_bn_bwd, bn_partial_fold_kernel)
BNP_MAX_BLOCKS, BNP_MAX_SLOTS = 1024, 8


def bnp_blocks(npix):
    return max(1, min(BNP_MAX_BLOCKS, -(-npix // 64)))


def bn_path(nch, scratch):
    """'wg' (one workgroup per channel: no scratch, misaligned scratch, C > 2048), 'small' (C <= 256: R = 256 / C rows per trip), 'slot'"""
    if scratch != "given" or nch > 256 * BNP_MAX_SLOTS:
        return "wg"
    return "small" if nch <= 256 else "slot"


def fold_branches(nb):
    """which branches of bn_partial_fold_kernel's loop over the nb partial rows run: slice sl walks rows sl, sl + 32, ... four at a
    time while k + 96 < nb, then one at a time"""
    got = set()
    for sl in range(32):
        k, nu, nr = sl, 0, 0
        while k + 96 < nb:
            k, nu = k + 128, nu + 1
        while k < nb:
            k, nr = k + 32, nr + 1
        got |= {"unrolled"} if nu else set()
        got |= {"remainder"} if nr else set()
        got |= {"unrolled+remainder"} if nu and nr else set()
        got |= {"idle slice"} if nu + nr == 0 else set()
    return got


def idle_workgroups(npix):
    nb = bnp_blocks(npix)
    per = -(-npix // nb)
    return sum(1 for b in range(nb) if b * per >= npix)


def nb_class(nb):
    return "1" if nb == 1 else "<32" if nb < 32 else "<128" if nb < 128 else "128" if nb == 128 else "1024" if nb == 1024 else "(128,1024)"


BN_C = (1, 3, 7, 96, 103, 199, 255, 256, 257, 300, 1024, 2048, 2049)
_NPIX_SMALL = (1, 50, 1000, 5000, 8192, 13000, 65537)        # nb = 1, 1, 16, 79, 128, 204, 1024 (the last 15 workgroups empty)
_NPIX_WIDE = (1, 37, 1000, 5000, 8192)


def _bn_cases():
    cases = []
    for c in BN_C:
        for n in (_NPIX_SMALL if c <= 300 else _NPIX_WIDE):
            cases.append((c, n, "given"))
        for n in ((1, 1000, 65537) if c <= 300 else (37, 5000)):
            cases += [(c, n, "null"), (c, n, "misaligned")]
    cases += [(96, 422400, "given"), (199, 422400, "given")]         # bench: npix = 32 x 600 x 22
    return cases


BN_CASES = _bn_cases()


def test_bn_case_table_reaches_every_path_and_fold_branch():
    seen = {(bn_path(c, s), nb_class(bnp_blocks(n))) for c, n, s in BN_CASES}
    for path in ("small", "slot"):
        for cls in ("1", "<32", "<128", "128", "(128,1024)", "1024"):
            assert (path, cls) in seen, (path, cls)
    assert {bn_path(c, s) for c, n, s in BN_CASES if s != "given"} == {"wg"}
    assert {s for c, n, s in BN_CASES if bn_path(c, s) == "wg"} == {"given", "null", "misaligned"}      # C = 2049 takes it with scratch
    for path in ("small", "slot"):
        branches = set().union(*(fold_branches(bnp_blocks(n)) for c, n, s in BN_CASES if bn_path(c, s) == path))
        assert branches == {"unrolled", "remainder", "unrolled+remainder", "idle slice"}, (path, branches)
        assert any(idle_workgroups(n) for c, n, s in BN_CASES if bn_path(c, s) == path)
        assert any(n == 1 for c, n, s in BN_CASES if bn_path(c, s) == path)
    assert idle_workgroups(65537) == 15 and bnp_blocks(65537) == 1024
    assert set(BN_C) == {c for c, _, _ in BN_CASES}
    slot_cs = {c for c, n, s in BN_CASES if bn_path(c, s) == "slot"}
    assert any(c % 256 for c in slot_cs) and 2048 in slot_cs                                   # a partial last slot and all eight slots
    assert any(256 % c for c, n, s in BN_CASES if bn_path(c, s) == "small")                     # threads beyond R rows idle
    assert {(96, 422400), (199, 422400)} <= {(c, n) for c, n, s in BN_CASES if s == "given"}


# ---- plumbing
@pytest.fixture(scope="module")
def stream():
    threads = torch.get_num_threads()
    torch.set_num_threads(min(16, threads))
    yield torch.cuda.Stream()
    torch.set_num_threads(threads)


def run(fn, *args, st):
    """enqueue on the side stream (after everything the default stream was given), wait for it, demand SELD_OK"""
    torch.cuda.synchronize()
    rc = fn(*args, C.c_void_p(st.cuda_stream))
    st.synchronize()
    assert rc == 0, f"{fn.__name__}: {rc}"


def nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def offset_data(gen, npix, nch, scale=1.0):
    """[npix, nch] fp32 on the device, channel c ~ N(3 + c / nch, scale^2)"""
    z = torch.randn((npix, nch), device="cuda", generator=gen) * scale
    return z + (3.0 + torch.arange(nch, device="cuda", dtype=torch.float32) / nch)


def within_fp32_rounding(name, got, ref, floor):
    """|got - ref| <= 2^-23 |ref| + floor, elementwise: one rounding of a double to fp32 (with a margin of one ulp for the order of the
    double sums), and `floor` for values near zero"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert np.isfinite(got).all(), name
    err = np.abs(got - ref)
    bar = 2.0 ** -23 * np.abs(ref) + floor
    worst = float((err / np.maximum(np.abs(ref), 1e-300)).max())
    print(f"[parity] {name:40s} max rel elementwise={worst:.3e}  (bar 2^-23 = {2.0 ** -23:.3e})")
    assert (err <= bar).all(), f"{name}: {int((err > bar).sum())} elements beyond one fp32 rounding; worst {float((err - bar).max()):.3e}"


def tensor_rel(name, got, ref, tol):
    check(name, got, ref)
    if tol < 1e-4:
        check(name + " (tight)", got, ref, tol=tol)


def within_ulps(name, got, ref32, ulps=1):
    got, ref32 = np.asarray(got, np.float32), np.asarray(ref32, np.float32)
    assert np.isfinite(got).all(), name
    d = np.abs(got.astype(np.float64) - ref32.astype(np.float64))
    bar = ulps * np.spacing(np.abs(ref32)).astype(np.float64)
    print(f"[parity] {name:40s} max |diff| / ulp = {float((d / np.maximum(bar, 1e-45)).max()):.3f}")
    assert (d <= bar).all(), f"{name}: beyond {ulps} ulp of the fp32 result"


def bitwise(name, got, ref):
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    assert got.shape == ref.shape, name
    ok = got.view(np.int32) == ref.view(np.int32)
    print(f"[parity] {name:40s} bit-identical elements {int(ok.sum())}/{ok.size}")
    assert ok.all(), f"{name}: {int((~ok).sum())} elements differ"


# ---- BatchNormalization
def _bn_scratch(lib, nch, mode):
    if mode == "null":
        return None, None
    buf = torch.empty(int(lib.seld_m_bn_scratch(nch)) + 2, device="cuda")
    addr = buf.data_ptr() + (4 if mode == "misaligned" else 0)
    return buf, C.c_void_p(addr)


@pytest.mark.parametrize("C_,npix,scr", BN_CASES, ids=[f"C{c}-n{n}-{s}" for c, n, s in BN_CASES])
def test_bn_stats_bwd_apply(seld_lib, stream, C_, npix, scr):
    lib = seld_lib
    gen = torch.Generator(device="cuda").manual_seed(C_ * 7919 + npix)
    z = offset_data(gen, npix, C_)
    dy = torch.randn((npix, C_), device="cuda", generator=gen) + (torch.arange(C_, device="cuda", dtype=torch.float32) / C_ - 0.5)
    gamma = torch.rand(C_, device="cuda", generator=gen) + 0.5
    beta = torch.randn(C_, device="cuda", generator=gen)
    sbuf, sp = _bn_scratch(lib, C_, scr)
    tag = f"C={C_} npix={npix} {scr} ({bn_path(C_, scr)}, nb={bnp_blocks(npix)})"
    eps = np.float32(1e-3)
    # stats, twice: the same bits
    outs = []
    for _ in range(2):
        mean, var = nan(C_), nan(C_)
        run(lib.seld_m_bn_stats, ptr(z), npix, C_, ptr(mean), ptr(var), sp, st=stream)
        outs.append((mean.cpu().numpy(), var.cpu().numpy()))
    bitwise(f"bn_stats mean repeat {tag}", outs[0][0], outs[1][0])
    bitwise(f"bn_stats var repeat {tag}", outs[0][1], outs[1][1])
    z64 = z.double().cpu()
    m_ref = z64.mean(0)
    v_ref = ((z64 - m_ref) ** 2).mean(0)
    check(f"bn_stats mean {tag}", outs[0][0], m_ref.numpy())
    check(f"bn_stats var {tag}", outs[0][1], v_ref.numpy())
    within_fp32_rounding(f"bn_stats mean {tag}", outs[0][0], m_ref.numpy(), 1e-30)
    # the variance is E[z^2] - mean^2 in double: a cancellation of ~|mean|^2 / var against 2^-53, far below one fp32 rounding
    within_fp32_rounding(f"bn_stats var {tag}", outs[0][1], v_ref.numpy(), 1e-12 * (m_ref.numpy() ** 2 + 1))
    mean, var = torch.as_tensor(outs[0][0], device="cuda"), torch.as_tensor(outs[0][1], device="cuda")
    # backward, twice, from the kernel's own fp32 mean / var
    outs = []
    for _ in range(2):
        dz, dg, db = nan(npix, C_), nan(C_), nan(C_)
        run(lib.seld_m_bn_bwd, ptr(z), ptr(dy), ptr(mean), ptr(var), ptr(gamma), C.c_float(eps), ptr(dz), ptr(dg), ptr(db), npix, C_, sp,
            st=stream)
        outs.append((dz.cpu().numpy(), dg.cpu().numpy(), db.cpu().numpy()))
    for i, n in enumerate(("dz", "dgamma", "dbeta")):
        bitwise(f"bn_bwd {n} repeat {tag}", outs[0][i], outs[1][i])
    mu, is_ = mean.double().cpu(), 1.0 / torch.sqrt(var.double().cpu() + float(eps))
    dy64 = dy.double().cpu()
    xh = (z64 - mu) * is_
    terms = dy64 * xh
    dg_ref, db_ref = terms.sum(0), dy64.sum(0)
    check(f"bn_bwd dgamma {tag}", outs[0][1], dg_ref.numpy())
    check(f"bn_bwd dbeta {tag}", outs[0][2], db_ref.numpy())
    within_fp32_rounding(f"bn_bwd dgamma {tag}", outs[0][1], dg_ref.numpy(), 1e-12 * terms.abs().sum(0).numpy())
    within_fp32_rounding(f"bn_bwd dbeta {tag}", outs[0][2], db_ref.numpy(), 1e-12 * dy64.abs().sum(0).numpy())
    dz_ref = gamma.double().cpu() * is_ * (dy64 - db_ref / npix - xh * dg_ref / npix)
    tensor_rel(f"bn_bwd dz {tag}", outs[0][0], dz_ref.numpy(), 1e-6)
    del dy64, terms, dz_ref
    # apply, both forms
    y_ref = (xh * gamma.double().cpu() + beta.double().cpu()).numpy()
    out = nan(npix, C_)
    run(lib.seld_m_bn_apply, ptr(z), ptr(mean), ptr(var), ptr(gamma), ptr(beta), C.c_float(eps), ptr(out), npix, C_, 0, st=stream)
    tensor_rel(f"bn_apply {tag}", out.cpu().numpy(), y_ref, 1e-6)
    prev = torch.randn((npix, C_), device="cuda", generator=gen)
    out = prev.clone()
    run(lib.seld_m_bn_apply, ptr(z), ptr(mean), ptr(var), ptr(gamma), ptr(beta), C.c_float(eps), ptr(out), npix, C_, 1, st=stream)
    tensor_rel(f"bn_apply accumulate {tag}", out.cpu().numpy(), prev.double().cpu().numpy() + y_ref, 1e-6)
    del sbuf


@pytest.mark.parametrize("C_,count", [(1, 1), (7, 1), (199, 422400), (2049, 65537), (300, 2)])
def test_bn_moving(seld_lib, stream, C_, count):
    gen = torch.Generator(device="cuda").manual_seed(C_ + count)
    mean = torch.randn(C_, device="cuda", generator=gen) + 3
    var = torch.rand(C_, device="cuda", generator=gen) * 2
    mm0, mv0 = torch.randn(C_, device="cuda", generator=gen), torch.rand(C_, device="cuda", generator=gen)
    mm, mv = mm0.clone(), mv0.clone()
    mom = np.float32(0.99)
    run(seld_lib.seld_m_bn_moving, ptr(mean), ptr(var), ptr(mm), ptr(mv), C_, C.c_float(mom), count, st=stream)
    unb = var.double().cpu() * (count / (count - 1) if count > 1 else 1.0)
    m64 = float(mom)
    tensor_rel(f"bn_moving mean C={C_} count={count}", mm.cpu().numpy(), (mm0.double().cpu() * m64 + mean.double().cpu() * (1 - m64)).numpy(), 1e-6)
    tensor_rel(f"bn_moving var C={C_} count={count}", mv.cpu().numpy(), (mv0.double().cpu() * m64 + unb * (1 - m64)).numpy(), 1e-6)


# ---- im2col / col2im (TensorFlow 'SAME')
def same_pads(n, k, s):
    out = -(-n // s)
    tot = max((out - 1) * s + k - n, 0)
    return out, tot // 2, tot - tot // 2


def im2col_ref(x, kh, kw, sh, sw):
    """x [B,H,W,C] (any dtype / device) -> [B*Ho*Wo, kh*kw*C]: zero padding, pad_before = total // 2"""
    B, H, W, Cc = x.shape
    Ho, ph0, ph1 = same_pads(H, kh, sh)
    Wo, pw0, pw1 = same_pads(W, kw, sw)
    xp = F.pad(x, (0, 0, pw0, pw1 + sw, ph0, ph1 + sh))
    cols = [xp[:, ki:ki + (Ho - 1) * sh + 1:sh, kj:kj + (Wo - 1) * sw + 1:sw, :] for ki in range(kh) for kj in range(kw)]
    return torch.stack(cols, 3).reshape(B * Ho * Wo, kh * kw * Cc)


def col2im_ref(y, shape, kh, kw, sh, sw):
    """the adjoint of im2col_ref, by explicit slice sums (y [B*Ho*Wo, kh*kw*C])"""
    B, H, W, Cc = shape
    Ho, ph0, ph1 = same_pads(H, kh, sh)
    Wo, pw0, pw1 = same_pads(W, kw, sw)
    y = y.reshape(B, Ho, Wo, kh, kw, Cc)
    xp = torch.zeros((B, H + ph0 + ph1 + sh, W + pw0 + pw1 + sw, Cc), dtype=y.dtype, device=y.device)
    for ki in range(kh):
        for kj in range(kw):
            xp[:, ki:ki + (Ho - 1) * sh + 1:sh, kj:kj + (Wo - 1) * sw + 1:sw, :] += y[:, :, :, ki, kj, :]
    return xp[:, ph0:ph0 + H, pw0:pw0 + W, :]


_CONV_SMALL = [(2, 9, 7, 3, k, k, s0, s1) for k in (1, 2, 3, 4, 5) for s0, s1 in ((1, 1), (2, 2), (1, 3), (3, 1), (5, 3))] + [
    (1, 2, 3, 2, 4, 5, 1, 1),       # k > H, k > W
    (2, 3, 4, 5, 2, 3, 4, 5),       # H < stride: Ho = Wo = 1, stride > k
    (3, 11, 1, 4, 3, 3, 2, 1),      # W = 1
    (1, 13, 5, 2, 2, 4, 3, 2),      # odd H / W with even kernels: the 'SAME' pads differ before / after
    (2, 1, 1, 6, 3, 3, 1, 1),       # a single pixel
]


@pytest.mark.parametrize("B,H,W,C_,kh,kw,sh,sw", _CONV_SMALL)
def test_im2col_col2im_small(seld_lib, stream, B, H, W, C_, kh, kw, sh, sw):
    lib = seld_lib
    gen = torch.Generator(device="cuda").manual_seed(H * 131 + W * 17 + kh * 5 + kw + sh * 3 + sw)
    x = offset_data(gen, B * H * W, C_).reshape(B, H, W, C_)
    Ho, Wo = -(-H // sh), -(-W // sw)
    K = kh * kw * C_
    col = nan(B * Ho * Wo, K)
    run(lib.seld_m_im2col, ptr(x), ptr(col), B, H, W, C_, kh, kw, sh, sw, st=stream)
    tag = f"{B,H,W,C_} k{kh,kw} s{sh,sw}"
    bitwise(f"im2col {tag}", col.cpu().numpy(), im2col_ref(x.cpu(), kh, kw, sh, sw).numpy())
    y = torch.randn((B * Ho * Wo, K), device="cuda", generator=gen)
    x64 = torch.zeros((B, H, W, C_), dtype=torch.float64, requires_grad=True)
    ref = torch.autograd.grad(im2col_ref(x64, kh, kw, sh, sw), x64, y.double().cpu())[0]
    sabs = torch.autograd.grad(im2col_ref(x64, kh, kw, sh, sw), x64, y.double().cpu().abs())[0]
    prev = torch.randn((B, H, W, C_), device="cuda", generator=gen)
    outs = []
    for acc in (0, 0, 1):
        dx = nan(B, H, W, C_) if not acc else prev.clone()
        run(lib.seld_m_col2im, ptr(y), ptr(dx), B, H, W, C_, kh, kw, sh, sw, acc, st=stream)
        outs.append(dx.cpu().numpy())
    bitwise(f"col2im repeat {tag}", outs[0], outs[1])
    _col2im_bar(f"col2im {tag}", outs[0], ref.numpy(), sabs.numpy())
    _col2im_bar(f"col2im accumulate {tag}", outs[2], prev.double().cpu().numpy() + ref.numpy(), sabs.numpy() + np.abs(prev.cpu().numpy()))


def _col2im_bar(name, got, ref, sabs):
    """elementwise: |got - ref| <= 1e-6 sum|terms| (at most kh kw fp32 additions of those terms)"""
    check(name, got, ref)
    err = np.abs(np.asarray(got, np.float64) - ref)
    worst = float((err / np.maximum(sabs, 1e-30)).max())
    print(f"[parity] {name:40s} max |err| / sum|terms| = {worst:.3e}")
    assert (err <= 1e-6 * sabs).all(), f"{name}: {worst:.3e}"


def _bench_convs():
    (in0, out0), (in1, out1) = bench_shapes()["blocks"]
    return [((BENCH_B,) + in0, 3, (5, 3)),        # mb0.c1
            ((BENCH_B,) + in0, 1, (5, 3)),        # mb0.p1_0 / s2_0: 1 x 1 with the strides
            ((BENCH_B,) + in1, 3, (1, 1))]        # mb1.c1 (its column matrix: 1.6 GB)


@pytest.mark.parametrize("i", range(3))
def test_im2col_col2im_bench_shapes(seld_lib, stream, i):
    """At the bench's shapes the references run as fp64 torch on the device (the mb1 column matrix is 1.6 GB): im2col bit for bit,
    col2im elementwise against the explicit slice sums, and the adjoint identity <col2im(y), x> = <y, im2col(x)> in fp64."""
    lib = seld_lib
    shape, k, (sh, sw) = _bench_convs()[i]
    B, H, W, C_ = shape
    gen = torch.Generator(device="cuda").manual_seed(100 + i)
    x = offset_data(gen, B * H * W, C_).reshape(shape)
    Ho, Wo = -(-H // sh), -(-W // sw)
    col = nan(B * Ho * Wo, k * k * C_)
    run(lib.seld_m_im2col, ptr(x), ptr(col), B, H, W, C_, k, k, sh, sw, st=stream)
    tag = f"bench {shape} k{k} s{sh,sw}"
    ok = bool(torch.equal(col, im2col_ref(x, k, k, sh, sw)))
    print(f"[parity] im2col {tag}: bit-identical {ok}")
    assert ok, tag
    y = torch.randn(col.shape, device="cuda", generator=gen)
    del col
    outs = []
    for _ in range(2):
        dx = nan(*shape)
        run(lib.seld_m_col2im, ptr(y), ptr(dx), B, H, W, C_, k, k, sh, sw, 0, st=stream)
        outs.append(dx)
    assert torch.equal(outs[0], outs[1]), f"col2im {tag}: not deterministic"
    dx = outs[0]
    ref = col2im_ref(y.double(), shape, k, k, sh, sw)
    sabs = col2im_ref(y.abs().double(), shape, k, k, sh, sw)
    err = (dx.double() - ref).abs()
    worst = float((err / sabs.clamp_min(1e-30)).max())
    print(f"[parity] col2im {tag}: max |err| / sum|terms| = {worst:.3e}, tensor rel = {float(err.max() / ref.abs().max()):.3e}")
    assert bool((err <= 1e-6 * sabs).all()) and float(err.max() / ref.abs().max()) <= 1e-4, tag
    del ref, err, sabs
    lhs = float((dx.double() * x.double()).sum())
    rhs, mag = _adjoint_by_taps(x, y, k, sh, sw)       # <y, im2col(x)> without the fp64 column matrix
    rel = abs(lhs - rhs) / mag
    print(f"[parity] col2im adjoint {tag}: |<col2im y, x> - <y, im2col x>| / <|y|, |im2col x|> = {rel:.3e}")
    assert rel <= 1e-6, tag


def _adjoint_by_taps(x, y, k, sh, sw):
    B, H, W, C_ = x.shape
    Ho, ph0, ph1 = same_pads(H, k, sh)
    Wo, pw0, pw1 = same_pads(W, k, sw)
    xp = F.pad(x, (0, 0, pw0, pw1 + sw, ph0, ph1 + sh))
    yv = y.reshape(B, Ho, Wo, k, k, C_)
    rhs = mag = 0.0
    for ki in range(k):
        for kj in range(k):
            p = yv[:, :, :, ki, kj, :].double() * xp[:, ki:ki + (Ho - 1) * sh + 1:sh, kj:kj + (Wo - 1) * sw + 1:sw, :].double()
            rhs += float(p.sum())
            mag += float(p.abs().sum())
    return rhs, mag


# ---- the fp32 MFMA GEMMs
GEMM_BAR = 2e-6      # |C - ref| / (|A| |B| + |bias|): see the docstring of test_gemm_small_m


def _gemm_case(lib, stream, gen, M, N, K, transb, bias_on, offset, accumulate, rows=None):
    """returns the magnitude-normalised error over `rows` (all rows when None)"""
    nA, nB = M * K + offset, N * K + offset
    Abuf = torch.randn(nA, device="cuda", generator=gen)
    Bbuf = torch.randn(nB, device="cuda", generator=gen) / math.sqrt(K)
    A = Abuf[offset:].view(M, K)
    Bm = Bbuf[offset:].view(N, K) if transb else Bbuf[offset:].view(K, N)
    bias = torch.randn(N, device="cuda", generator=gen) if bias_on else None
    C0 = torch.randn((M, N), device="cuda", generator=gen) if accumulate else nan(M, N)
    Cm = C0.clone()
    run(lib.seld_m_gemm, ptr(A), ptr(Bm), ptr(bias), ptr(Cm), M, N, K, transb, accumulate, st=stream)
    idx = torch.arange(M, device="cuda") if rows is None else rows
    a = A[idx].double().cpu()
    b = (Bm.t() if transb else Bm).double().cpu()
    ref = a @ b
    mag = a.abs() @ b.abs()
    if bias is not None:
        ref, mag = ref + bias.double().cpu(), mag + bias.double().cpu().abs()
    if accumulate:
        ref, mag = ref + C0[idx].double().cpu(), mag + C0[idx].double().cpu().abs()
    got = Cm[idx].double().cpu()
    assert bool(torch.isfinite(got).all())
    check(f"gemm M={M} N={N} K={K} tb={transb} bias={int(bias_on)} off={offset} acc={accumulate}", got.numpy(), ref.numpy())
    return float(((got - ref).abs() / mag.clamp_min(1e-30)).max())


@pytest.mark.parametrize("M", [1, 65])
@pytest.mark.parametrize("transb", [0, 1])
@pytest.mark.parametrize("K", [1, 3, 63, 927, 4378])
def test_gemm_small_m(seld_lib, stream, M, transb, K):
    """C = A op(B) + bias (+C) for every N in the list, with / without bias, offset-by-one-float operands (the scalar-load path) and
    the accumulating form.  The bar: the fp32 MFMA takes exact products and accumulates in fp32, K / 2 steps per chain, so the error is
    a sum of K roundings of partial sums bounded by |A| |B|; 2e-6 of |A| |B| + |bias| is the bar of test_gemm_split_bf16."""
    gen = torch.Generator(device="cuda").manual_seed(M * 10 + transb + K)
    worst = 0.0
    for j, N in enumerate((1, 7, 63, 65, 96, 384, 927, 4378)):
        e = _gemm_case(seld_lib, stream, gen, M, N, K, transb, bias_on=j % 2 == 0, offset=j % 3 == 1, accumulate=0)
        e = max(e, _gemm_case(seld_lib, stream, gen, M, N, K, transb, bias_on=j % 2 == 1, offset=j % 3 == 2, accumulate=1))
        worst = max(worst, e)
    print(f"[parity] gemm M={M} tb={transb} K={K}: max |C - ref| / (|A||B| + |bias|) = {worst:.3e}")
    assert worst <= GEMM_BAR


# (M, N, K, transb): the bench's module products (mb0.c1 and its input gradient, mb0's 1x1 projections, mb1.c1 and its input gradient,
# the GRU's input projection and input gradient), plus ragged offset forms
_GEMM_BENCH = [(422400, 96, 63, 0, 0), (422400, 63, 96, 1, 0), (422400, 96, 7, 0, 0), (422400, 7, 7, 0, 1), (422400, 96, 927, 0, 0),
               (422400, 927, 96, 1, 1), (19200, 384, 4378, 0, 0), (19200, 4378, 384, 1, 0), (19200, 65, 63, 0, 1), (19200, 96, 927, 1, 1)]


@pytest.mark.parametrize("M,N,K,transb,offset", _GEMM_BENCH)
def test_gemm_bench_shapes(seld_lib, stream, M, N, K, transb, offset):
    """Rows sampled with a stride, plus the first and last 64-row tiles, against fp64 on those rows."""
    gen = torch.Generator(device="cuda").manual_seed(M + N + K)
    rows = torch.unique(torch.cat([torch.arange(64), torch.arange(0, M, 211 if M > 100000 else 37), torch.arange(M - 64, M)])).cuda()
    e = _gemm_case(seld_lib, stream, gen, M, N, K, transb, bias_on=transb == 0, offset=offset, accumulate=0, rows=rows)
    print(f"[parity] gemm bench M={M} N={N} K={K} tb={transb}: max |C - ref| / (|A||B| + |bias|) = {e:.3e}")
    assert e <= GEMM_BAR


_TN_CASES = [(1, 1, 1, 0, 0), (65, 3, 7, 0, 0), (1000, 63, 65, 0, 0), (4096, 927, 96, 0, 0), (422400, 927, 96, 0, 0), (422400, 63, 96, 0, 0),
             (422400, 7, 7, 0, 0), (19200, 4378, 384, 0, 0), (19200, 128, 384, 600, 1), (19200, 128, 384, 600, -1), (2100, 128, 384, 7, 1),
             (2100, 128, 384, 7, -1), (7, 5, 3, 7, 1)]


@pytest.mark.parametrize("M,K1,N,seq,shift", _TN_CASES)
def test_gemm_tn(seld_lib, stream, M, K1, N, seq, shift):
    """C = A_shift^T B (+ colsum B) with the slab reduction, twice (same bits); the fp64 reference runs as torch on the device.  seq /
    shift: row m of A replaced by row m + shift of its length-seq sequence, zero outside (a GRU direction's recurrent-kernel gradient)."""
    lib = seld_lib
    gen = torch.Generator(device="cuda").manual_seed(M + K1 + N + seq + shift)
    A = offset_data(gen, M, K1)
    Bm = torch.randn((M, N), device="cuda", generator=gen)
    slab = torch.empty(int(lib.seld_m_gemm_tn_scratch(K1, N)), device="cuda")
    outs = []
    for with_cs in (1, 1, 0):
        Cm, cs = nan(K1, N), (nan(N) if with_cs else None)
        run(lib.seld_m_gemm_tn, ptr(A), ptr(Bm), ptr(Cm), ptr(cs), ptr(slab), M, K1, N, seq, shift, st=stream)
        outs.append((Cm, cs))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "gemm_tn: not deterministic"
    assert torch.equal(outs[0][0], outs[2][0]), "gemm_tn: the colsum changes the product"
    A64 = A.double()
    if seq:
        t = torch.arange(M, device="cuda") % seq
        src = torch.arange(M, device="cuda") + shift
        okm = ((t + shift) >= 0) & ((t + shift) < seq)
        A64 = torch.where(okm[:, None], A64[src.clamp(0, M - 1)], torch.zeros_like(A64))
    ref = A64.t() @ Bm.double()
    mag = A64.abs().t() @ Bm.double().abs()
    got = outs[0][0].double()
    tag = f"gemm_tn M={M} K1={K1} N={N} seq={seq} shift={shift}"
    check(tag, got.cpu().numpy(), ref.cpu().numpy())
    e = float(((got - ref).abs() / mag.clamp_min(1e-30)).max())
    print(f"[parity] {tag}: max |C - ref| / (|A||B|) = {e:.3e}")
    assert e <= GEMM_BAR
    cs_ref = Bm.double().sum(0)
    check(tag + " colsum", outs[0][1].cpu().numpy(), cs_ref.cpu().numpy())
    ecs = float(((outs[0][1].double() - cs_ref).abs() / Bm.double().abs().sum(0)).max())
    print(f"[parity] {tag} colsum: max |err| / sum|B| = {ecs:.3e}")
    assert ecs <= GEMM_BAR
    if seq > 1:          # rows that do not tile into sequences: refused, nothing enqueued
        assert lib.seld_m_gemm_tn(ptr(A), ptr(Bm), ptr(outs[0][0]), None, ptr(slab), M - 1, K1, N, seq, shift, C.c_void_p(stream.cuda_stream)) == -1


# ---- activations
_ACT_X = [0.0, -0.0, 1e-30, -1e-30, 1.0, -1.0, 20.0, -20.0, 100.0, -100.0]


def _act_ref(x, kind):
    s = torch.sigmoid(x)
    y = [x, s, torch.tanh(x), torch.relu(x), x * s][kind]
    d = [torch.ones_like(x), s * (1 - s), 1 - torch.tanh(x) ** 2, (x > 0).to(x.dtype), s + x * s * (1 - s)][kind]
    return y, d


@pytest.mark.parametrize("kind", range(5))
def test_act(seld_lib, stream, kind):
    gen = torch.Generator(device="cuda").manual_seed(kind)
    x = torch.cat([torch.tensor(_ACT_X, device="cuda"), torch.randn(100003, device="cuda", generator=gen) * 4])
    n = x.numel()
    dy = torch.randn(n, device="cuda", generator=gen)
    prev = torch.randn(n, device="cuda", generator=gen)
    y = nan(n)
    run(seld_lib.seld_m_act, ptr(x), ptr(y), n, kind, st=stream)
    dx0, dx1 = nan(n), prev.clone()
    run(seld_lib.seld_m_act_bwd, ptr(x), ptr(dy), ptr(dx0), n, kind, 0, st=stream)
    run(seld_lib.seld_m_act_bwd, ptr(x), ptr(dy), ptr(dx1), n, kind, 1, st=stream)
    x32, dy32, p32 = x.cpu().numpy(), dy.cpu().numpy(), prev.cpu().numpy()
    got = [y.cpu().numpy(), dx0.cpu().numpy(), dx1.cpu().numpy()]
    assert all(np.isfinite(g).all() for g in got), "non-finite activation output"
    if kind in (0, 3):              # linear, relu: exact in fp32
        yr = x32 if kind == 0 else np.maximum(x32, np.float32(0))
        dr = dy32 * (np.float32(1) if kind == 0 else (x32 > 0).astype(np.float32))
        bitwise(f"act kind {kind}", got[0], yr)
        bitwise(f"act_bwd kind {kind}", got[1], dr)
        bitwise(f"act_bwd accumulate kind {kind}", got[2], p32 + dr)
        return
    y64, d64 = _act_ref(torch.as_tensor(x32, dtype=torch.float64), kind)
    g64 = torch.as_tensor(dy32, dtype=torch.float64) * d64
    for name, g, r in ((f"act kind {kind}", got[0], y64), (f"act_bwd kind {kind}", got[1], g64),
                       (f"act_bwd accumulate kind {kind}", got[2], g64 + torch.as_tensor(p32, dtype=torch.float64))):
        r = r.numpy()
        check(name, g, r)
        e = float((np.abs(g - r) / np.maximum(1.0, np.abs(r))).max())
        print(f"[parity] {name:40s} max |err| / max(1, |ref|) = {e:.3e}")
        # swish': s + x s (1 - s), and 1 - s of an fp32 s near 1 is a multiple of 2^-24: x dy 2^-24 more (measured without it: 1.24e-6)
        extra = 2.0 ** -24 * np.abs(x32.astype(np.float64) * dy32) if kind == 4 and "bwd" in name else 0.0
        assert (np.abs(g - r) <= 1e-6 * np.maximum(1.0, np.abs(r)) + extra).all(), name


# ---- elementwise pieces: axpy, copy_channels, the squeeze-and-excitation operators
def test_axpy(seld_lib, stream):
    gen = torch.Generator(device="cuda").manual_seed(5)
    for n, alpha in ((1, 1.0), (1000, -0.37), (422400 * 7 + 3, 1.0)):
        dst0, src = torch.randn(n, device="cuda", generator=gen) + 3, torch.randn(n, device="cuda", generator=gen)
        dst = dst0.clone()
        run(seld_lib.seld_m_axpy, ptr(dst), ptr(src), n, C.c_float(alpha), st=stream)
        within_ulps(f"axpy n={n} alpha={alpha}", dst.cpu().numpy(), dst0.cpu().numpy() + np.float32(alpha) * src.cpu().numpy())


@pytest.mark.parametrize("rows,Cs,Cd,off", [(4224, 7, 103, 0), (4224, 96, 103, 7), (4224, 103, 199, 0), (422400, 96, 199, 103),
                                            (4224, 50, 199, 70), (1, 1, 1, 0), (333, 3, 5, 1)])
def test_copy_channels(seld_lib, stream, rows, Cs, Cd, off):
    gen = torch.Generator(device="cuda").manual_seed(rows + Cs + off)
    src = offset_data(gen, rows, Cs)
    dst = torch.randn((rows, Cd), device="cuda", generator=gen)
    d0 = dst.cpu().numpy()
    run(seld_lib.seld_m_copy_channels, ptr(src), ptr(dst), rows, Cs, Cd, off, 0, st=stream)
    want = d0.copy()
    want[:, off:off + Cs] = src.cpu().numpy()
    bitwise(f"copy_channels mode 0 rows={rows} {Cs}->{Cd}@{off}", dst.cpu().numpy(), want)
    s0 = src.cpu().numpy()
    run(seld_lib.seld_m_copy_channels, ptr(src), ptr(dst), rows, Cs, Cd, off, 1, st=stream)
    within_ulps(f"copy_channels mode 1 rows={rows} {Cs}<-{Cd}@{off}", src.cpu().numpy(), s0 + want[:, off:off + Cs])
    bitwise(f"copy_channels mode 1 leaves dst rows={rows}", dst.cpu().numpy(), want)


_SE_CASES = [(1, 1, 1), (2, 255, 3), (3, 256, 96), (2, 257, 103), (32, 13200, 199), (32, 1, 199), (4, 13200, 7)]


@pytest.mark.parametrize("B,HW,C_", _SE_CASES)
def test_squeeze_excitation_ops(seld_lib, stream, B, HW, C_):
    lib = seld_lib
    gen = torch.Generator(device="cuda").manual_seed(B * HW + C_)
    x = offset_data(gen, B * HW, C_).reshape(B, HW, C_)
    dy = torch.randn((B, HW, C_), device="cuda", generator=gen) + 0.25
    s = torch.rand((B, C_), device="cuda", generator=gen)
    tag = f"B={B} HW={HW} C={C_}"
    x64, dy64 = x.double().cpu(), dy.double().cpu()
    outs = []
    for _ in range(2):
        m, ds = nan(B, C_), nan(B, C_)
        run(lib.seld_m_mean_hw, ptr(x), ptr(m), B, HW, C_, st=stream)
        run(lib.seld_m_scale_hw_bwd_ds, ptr(x), ptr(dy), ptr(ds), B, HW, C_, st=stream)
        outs.append((m.cpu().numpy(), ds.cpu().numpy()))
    bitwise(f"mean_hw repeat {tag}", outs[0][0], outs[1][0])
    bitwise(f"scale_hw_bwd_ds repeat {tag}", outs[0][1], outs[1][1])
    m_ref = x64.mean(1).numpy()
    ds_ref = (dy64 * x64).sum(1)
    check(f"mean_hw {tag}", outs[0][0], m_ref)
    check(f"scale_hw_bwd_ds {tag}", outs[0][1], ds_ref.numpy())
    within_fp32_rounding(f"mean_hw {tag}", outs[0][0], m_ref, 1e-30)
    within_fp32_rounding(f"scale_hw_bwd_ds {tag}", outs[0][1], ds_ref.numpy(), 1e-12 * (dy64 * x64).abs().sum(1).numpy())
    y = nan(B, HW, C_)
    run(lib.seld_m_scale_hw, ptr(x), ptr(s), ptr(y), B, HW, C_, st=stream)
    within_ulps(f"scale_hw {tag}", y.cpu().numpy(), x.cpu().numpy() * s.cpu().numpy()[:, None, :])
    dmean = torch.randn((B, C_), device="cuda", generator=gen)
    prev = torch.randn((B, HW, C_), device="cuda", generator=gen)
    base = dy64 * s.double().cpu()[:, None, :]
    for dm, acc in ((None, 0), (dmean, 0), (dmean, 1), (None, 1)):
        dx = prev.clone() if acc else nan(B, HW, C_)
        run(lib.seld_m_scale_hw_bwd_dx, ptr(dy), ptr(s), ptr(dm), ptr(dx), B, HW, C_, acc, st=stream)
        ref = base + (dm.double().cpu()[:, None, :] / HW if dm is not None else 0) + (prev.double().cpu() if acc else 0)
        tensor_rel(f"scale_hw_bwd_dx dmean={dm is not None} acc={acc} {tag}", dx.cpu().numpy(), ref.numpy(), 1e-6)


# ---- the recurrent block, the losses and Adam: the seld_k_* kernels on the caller's stream
@pytest.mark.parametrize("B,S", [(1, 1), (2, 7), (32, 600)])
def test_gru_stream_form_matches_k_form(seld_lib, stream, B, S):
    from test_kernels_gpu import _gru_ref
    lib = seld_lib
    rng = np.random.default_rng(B * 1000 + S)
    mk = lambda *s, sc=1.0: (rng.standard_normal(s) * sc).astype(np.float32)
    d = {k: dev(v) for k, v in dict(gxf=mk(B, S, 384), gxb=mk(B, S, 384), Uf=mk(128, 384, sc=1 / np.sqrt(128)), Ub=mk(128, 384, sc=1 / np.sqrt(128)),
                                    bf=mk(384, sc=0.1), bb=mk(384, sc=0.1), dout=mk(B, S, 128)).items()}
    res = {}
    for form in ("k", "m"):
        h_f, h_b, o, sv_f, sv_b = nan(B, S, 128), nan(B, S, 128), nan(B, S, 128), nan(B, S, 4, 128), nan(B, S, 4, 128)
        dgx_f, dgx_b, dgh_f, dgh_b = nan(B, S, 384), nan(B, S, 384), nan(B, S, 384), nan(B, S, 384)
        fa = [ptr(d[k]) for k in ("gxf", "gxb", "Uf", "Ub", "bf", "bb")] + [ptr(h_f), ptr(h_b), ptr(sv_f), ptr(sv_b), ptr(o), B, S, 128]
        ba = [ptr(d["dout"]), ptr(h_f), ptr(h_b), ptr(sv_f), ptr(sv_b), ptr(d["Uf"]), ptr(d["Ub"]), ptr(dgx_f), ptr(dgx_b), ptr(dgh_f), ptr(dgh_b),
              B, S, 128]
        if form == "k":
            assert lib.seld_k_gru_fwd(*fa) == 0 and lib.seld_k_gru_bwd(*ba) == 0
            torch.cuda.synchronize()
        else:
            run(lib.seld_m_gru_fwd, *fa, st=stream)
            run(lib.seld_m_gru_bwd, *ba, st=stream)
        res[form] = [t.cpu().numpy() for t in (h_f, h_b, o, sv_f, sv_b, dgx_f, dgx_b, dgh_f, dgh_b)]
    for i, name in enumerate(("h_f", "h_b", "out", "saved_f", "saved_b", "dgx_f", "dgx_b", "dgh_f", "dgh_b")):
        bitwise(f"gru_{'fwd' if i < 5 else 'bwd'} {name} m vs k {B,S}", res["m"][i], res["k"][i])
    tg = [torch.as_tensor(d[k].cpu().numpy(), dtype=torch.float64).requires_grad_(True) for k in ("gxf", "gxb")]
    tU = [torch.as_tensor(d[k].cpu().numpy(), dtype=torch.float64) for k in ("Uf", "Ub")]
    tb = [torch.as_tensor(d[k].cpu().numpy(), dtype=torch.float64) for k in ("bf", "bb")]
    hf, hb = _gru_ref(tg[0], tU[0], tb[0], False), _gru_ref(tg[1], tU[1], tb[1], True)
    g = torch.autograd.grad(hf * hb, tg, torch.as_tensor(d["dout"].cpu().numpy(), dtype=torch.float64))
    check(f"gru_fwd out {B,S}", res["m"][2], (hf * hb).detach().numpy())
    check(f"gru_bwd dgx_f {B,S}", res["m"][5], g[0].numpy())
    check(f"gru_bwd dgx_b {B,S}", res["m"][6], g[1].numpy())
    for units in (64, 256):
        assert lib.seld_m_gru_fwd(*([None] * 11), B, S, units, C.c_void_p(stream.cuda_stream)) == -2


@pytest.mark.parametrize("B,S", [(1, 1), (2, 7), (32, 600)])
@pytest.mark.parametrize("mode,den", [("MSE", 0.0), ("MMSE", 0.0), ("MMSE", 2.5)])
def test_losses_stream_form_matches_k_form(seld_lib, stream, B, S, mode, den):
    from seld_amd import _lib
    from oracle import seldnet_oracle as O
    lib, nc = seld_lib, 12
    rng = np.random.default_rng(B + S)
    _, ys, yd = O.synthetic_batch(B, S * 5, seed=11)
    sp, dp = rng.standard_normal((B, S, nc)) * 3, rng.standard_normal((B, S, 3 * nc))
    tsp = torch.as_tensor(sp, dtype=torch.float64).requires_grad_(True)
    tdp = torch.as_tensor(dp, dtype=torch.float64).requires_grad_(True)
    sed, doa = torch.sigmoid(tsp), torch.tanh(tdp)
    cfg = _lib.LossCfg(0 if mode == "MSE" else 1, 1.0, 1000.0, 1.0, den)
    sedd, doad, ysd, ydd = dev(sed.detach().numpy()), dev(doa.detach().numpy()), dev(ys), dev(yd)
    nd = B * S if mode == "MSE" else 1
    res = {}
    for form in ("k", "m"):
        sl, dl, gs, gd = nan(1), nan(nd), nan(B, S, nc), nan(B, S, 3 * nc)
        if form == "k":
            assert lib.seld_k_losses(ptr(sedd), ptr(doad), ptr(ysd), ptr(ydd), C.byref(cfg), ptr(sl), ptr(dl), ptr(gs), ptr(gd), B, S, nc) == 0
            torch.cuda.synchronize()
        else:
            scr = torch.empty(int(lib.seld_m_losses_scratch(B * S)), device="cuda")
            run(lib.seld_m_losses, ptr(sedd), ptr(doad), ptr(ysd), ptr(ydd), C.byref(cfg), ptr(sl), ptr(dl), ptr(gs), ptr(gd), ptr(scr), B, S, nc,
                st=stream)
        res[form] = [t.cpu().numpy() for t in (sl, dl, gs, gd)]
    for i, name in enumerate(("sloss", "dloss", "dsed_pre", "ddoa_pre")):
        bitwise(f"losses {mode} den={den} {name} m vs k {B,S}", res["m"][i], res["k"][i])
    if den == 0.0:       # the fp64 oracle computes the denominator from the labels: the bars of test_kernels_gpu.py::test_losses
        # from the fp32 head outputs the kernels read, through d sigmoid = p (1 - p), d tanh = 1 - d^2 of those outputs: near p = 1 the
        # fp32 p itself moves 1 - p by 2^-24, and the BCE's (1 - p) / (1 - p + 1e-7) with it (5e-3 of the largest gradient at (32, 600))
        p = torch.as_tensor(sedd.cpu().numpy(), dtype=torch.float64).requires_grad_(True)
        q = torch.as_tensor(doad.cpu().numpy(), dtype=torch.float64).requires_grad_(True)
        obj, sl, dl = O.losses_and_objective(p, q, torch.as_tensor(ys, dtype=torch.float64), torch.as_tensor(yd, dtype=torch.float64), mode,
                                             (1.0, 1000.0))
        gp, gq = torch.autograd.grad(obj, (p, q))
        gs, gd = gp * p.detach() * (1 - p.detach()), gq * (1 - q.detach() ** 2)
        check(f"losses {mode} sloss {B,S}", res["m"][0], sl.detach().numpy().reshape(1))
        check(f"losses {mode} dloss {B,S}", res["m"][1], dl.detach().numpy().reshape(-1))
        check(f"losses {mode} dsed_pre {B,S}", res["m"][2], gs.numpy(), tol=2e-4)
        check(f"losses {mode} ddoa_pre {B,S}", res["m"][3], gd.numpy())


@pytest.mark.parametrize("n,step", [(1, 1), (10007, 3), (4378 * 384, 50)])
def test_adam_stream_form_matches_k_form(seld_lib, stream, n, step):
    from oracle import seldnet_oracle as O
    rng = np.random.default_rng(n)
    th, g, m, v = (rng.standard_normal(n).astype(np.float32) for _ in range(4))
    v = np.abs(v)
    res = {}
    for form in ("k", "m"):
        td, gd, md, vd = dev(th), dev(g), dev(m), dev(v)
        args = [ptr(td), ptr(gd), ptr(md), ptr(vd), n, 1e-3, 0.9, 0.999, 1e-7, step]
        if form == "k":
            assert seld_lib.seld_k_adam(*args) == 0
            torch.cuda.synchronize()
        else:
            run(seld_lib.seld_m_adam, *args, st=stream)
        res[form] = [t.cpu().numpy() for t in (td, md, vd)]
    for i, name in enumerate(("theta", "m", "v")):
        bitwise(f"adam {name} m vs k n={n}", res["m"][i], res["k"][i])
    rt, rm, rv = O.adam_update(*(torch.as_tensor(a, dtype=torch.float64) for a in (th, g, m, v)), step=step, lr=1e-3)
    for i, (name, r) in enumerate((("theta", rt), ("m", rm), ("v", rv))):
        check(f"adam {name} n={n} step={step}", res["m"][i], r.numpy(), tol=1e-6)


def test_every_module_operator_is_called_here():
    import os
    import re
    here = open(os.path.abspath(__file__)).read()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "seld_hip.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(seld_m_[a-z0-9_]+)\s*\(", hdr)))
    assert len(names) >= 24
    for n in names:
        if n == "seld_m_conv_out":
            continue            # a host function: tests/test_module_ops_cpu.py::test_conv_out_is_same_out
        assert re.search(r"lib\.%s\b" % n, here), f"{n} is not called in this file"
