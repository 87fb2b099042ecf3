"""Cases, seeded inputs and plain fp64 references for the GEMM family: gemm.hip (gemm_f32_kernel, gemm_tn_kernel, the slab reductions, heads_weff /
heads_grad, mul), gemm_sb.hip (gemm_sb_kernel, gemm_sb16_kernel, the weight split), gemm_tn_sb.hip and prep.hip.  Shared by
tests/test_gemm_family_cpu.py (conditions the cases and bars meet, without a GPU) and tests/test_gemm_family_gpu.py (the kernels).  Checker only.

Inputs are float32 before anything is computed from them, cached and read-only.  Operands of the products span thirteen binades (a normal variate times
2^[-6, 6], as test_gemm_split_bf16 draws them), so the mid and lo planes of a split carry weight.

Bars (all from the project):
  helpers.check, 1e-4 tensor-normalised: every tensor.
  BAR6 = 2e-6 on |C - ref| / (|A| |B| + |bias|): the fp32 MFMA kernels and the six-product split-bf16 kernels (GEMM_BAR of test_module_ops_gpu.py,
      the bound of test_gemm_split_bf16), with or without an activation; with accumulate the denominator also holds |C before| (_gemm_case of
      test_module_ops_gpu.py).  The BatchNorm partials of stat_part meet it against the fp64 sums of the stored rows, over sum |v| and sum v^2.
  BAR1 = 2e-6 tensor-normalised against the fp64 product of the bf16-rounded operands: bf16 single-product mode (test_bf16_single_product_conv64).
  BAR4 = FOUR_EMUL + 2e-6: the four-product form.  FOUR_EMUL is the largest magnitude-normalised error, over the inputs of every four-product case
      below, of the form's exact arithmetic (two planes per operand with the rounded mid of sb_tile.h split2r_pair, four products, fp64
      accumulation) against the fp64 product; test_gemm_family_cpu.py::test_four_product_emulation measures it and holds it under the constant."""
import functools
from collections import namedtuple

import numpy as np

from aux_kernel_cases import report, report_exact      # noqa: F401  (one reporting style for the per-kernel files)

BAR6 = 2e-6
BAR1 = 2e-6
# measured by test_four_product_emulation over four_cases() (the [four] lines it prints): the largest is 2.872e-5 (the kernel gradient of the 256-channel
# convolution on a 1 x 2 x 2 image: four-term sums, where nothing averages out), the single-row products follow at 2.6e-5, the K >= 128 products stay
# below 1e-5.  Two operands with 16 significant bits each, the second plane rounded, allow 2 * 2^-16 = 3.1e-5 at worst.
FOUR_EMUL = 2.9e-5
BAR4 = FOUR_EMUL + 2e-6
assert BAR4 < 1e-4


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def binade(rng, shape, lo=-6, hi=7):
    return (rng.standard_normal(shape) * np.exp2(rng.integers(lo, hi, size=shape))).astype(np.float32)


def f64(a):
    return np.asarray(a, np.float64)


def act64(x, act):
    if act == 1:
        with np.errstate(over="ignore"):      # exp(-x) = inf gives the sigmoid's 0
            return 1.0 / (1.0 + np.exp(-x))
    if act == 2:
        return np.tanh(x)
    if act == 3:
        return np.maximum(x, 0.0)
    return x


def act32(x, act):
    x = np.asarray(x, np.float32)
    if act == 1:
        with np.errstate(over="ignore"):
            return (np.float32(1) / (np.float32(1) + np.exp(-x))).astype(np.float32)
    if act == 2:
        return np.tanh(x).astype(np.float32)
    if act == 3:
        return np.maximum(x, np.float32(0))
    return x


def opb(B, transb):
    return B.T if transb else B


def product(A, B, transb=0, bias=None, act=0, prev=None, A1=None, B1=None):
    """(fp64 reference, magnitude denominator) of act(A op(B) [+ A1 op(B1)] + bias) [+ prev]"""
    ref = f64(A) @ f64(opb(B, transb))
    mag = np.abs(f64(A)) @ np.abs(f64(opb(B, transb)))
    if A1 is not None:
        ref = ref + f64(A1) @ f64(opb(B1, transb))
        mag = mag + np.abs(f64(A1)) @ np.abs(f64(opb(B1, transb)))
    if bias is not None:
        ref = ref + f64(bias)
        mag = mag + np.abs(f64(bias))
    ref = act64(ref, act)
    if prev is not None:
        ref = ref + f64(prev)
        mag = mag + np.abs(f64(prev))
    return ref, mag


def matmul32(A, B):
    """A @ B in float32 with nothing but elementwise numpy operations: every product rounded to float32, then summed pairwise over k.  Unlike the
    `@` of a BLAS, whose blocking and summation order depend on the machine, this gives the same bits everywhere"""
    P_ = np.asarray(A, np.float32)[:, :, None] * np.asarray(B, np.float32)[None, :, :]
    while P_.shape[1] > 1:
        if P_.shape[1] & 1:
            P_ = np.concatenate([P_, np.zeros_like(P_[:, :1])], axis=1)
        P_ = P_[:, 0::2] + P_[:, 1::2]
    return P_[:, 0]


def product32(A, B, transb=0, bias=None, act=0, prev=None, A1=None, B1=None):
    """the same in plain float32 numpy"""
    out = matmul32(A, opb(B, transb))
    if A1 is not None:
        out = out + matmul32(A1, opb(B1, transb))
    if bias is not None:
        out = out + np.asarray(bias, np.float32)
    out = act32(out, act)
    if prev is not None:
        out = out + np.asarray(prev, np.float32)
    return out


def mag_err(got, ref, mag):
    """largest |got - ref| / mag; an element of zero magnitude must be exact"""
    d = np.abs(f64(got) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(mag > 0, d / mag, np.where(d == 0, 0.0, np.inf))
    return float(e.max())


# ---------------------------------------------------------------- bf16 planes (sb_tile.h)
def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _from_bits(u):
    return np.asarray(u, np.uint32).view(np.float32)


def two_planes_rounded(x):
    """hi + mid of split2r_pair / split3(round_mid): hi = the upper 16 bits, mid = the residual with 0x8000 added to its bits, upper 16 bits"""
    x = np.ascontiguousarray(x, np.float32)
    hi = _from_bits(_bits(x) & np.uint32(0xffff0000))
    r = (x - hi).astype(np.float32)                          # exact
    mid = _from_bits((_bits(r) + np.uint32(0x8000)) & np.uint32(0xffff0000))
    return f64(hi) + f64(mid)


def bf16_rne(x):
    """round-to-nearest-even bf16 (common.h bf16_rne_bits), as float64"""
    u = _bits(x).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return f64(_from_bits(u.astype(np.uint32)))


# ---------------------------------------------------------------- gemm_f32_kernel
F32Case = namedtuple("F32Case", "M N K transb ld")
F32_MS, F32_NS, F32_KS = (1, 63, 64, 65), (1, 63, 65, 130), (1, 31, 32, 33, 67)
F32_LDS = ("tight", "pad4", "pad1", "off1")      # pad4: lda K + 4, ldb + 4 (the vector loads when K % 4 == 0); pad1: + 1 (scalar); off1: bases one float off 16 bytes


def _f32_cross():
    """twenty of the eighty combinations per transb: every value of every axis, every leading-dimension form, K = 32 under tight and pad4"""
    out = []
    for tb in (0, 1):
        for i in range(20):
            out.append(F32Case(F32_MS[i % 4], F32_NS[(i + i // 4 + tb) % 4], F32_KS[i % 5], tb, F32_LDS[(i + i // 4) % 4]))
    return tuple(out)


F32_CROSS = _f32_cross()
# no N of the cross is a multiple of 4: B's float4 loads under a padded ldb with transb = 0 need a case of their own
F32_CASES = F32_CROSS + (F32Case(65, 64, 32, 0, "pad4"),)
F32_EPI_SHAPES = ((64, 64, 32, 64), (65, 130, 33, 132))      # (M, N, K, ldc): whole tiles through the dwordx4 stores, and a mix of both store paths
F32_HEADS = ((12, 36), (1, 1), (70, 5), (64, 64))             # the split inside a tile, at the smallest, past the first tile, on a tile edge
F32_STAT = (130, 128, 33)                                     # three row blocks, the last of two rows


def f32_id(c):
    return f"M{c.M}-N{c.N}-K{c.K}-tb{c.transb}-{c.ld}"


def f32_lds(c):
    """(lda, ldb, ldc, extra floats in front of A and B)"""
    nat = c.K if c.transb else c.N
    if c.ld == "pad4":
        return c.K + 4, nat + 4, c.N + 3, 0
    if c.ld == "pad1":
        return c.K + 1, nat + 1, c.N + 3, 0
    if c.ld == "off1":
        return c.K, nat, c.N, 1
    return c.K, nat, c.N, 0


@functools.lru_cache(maxsize=None)
def f32_inputs(M, N, K, transb, seed=3):
    """A, B, bias, the C before an accumulate, and a second pair A1, B1 / bias1"""
    rng = np.random.default_rng([seed, M, N, K, transb])
    bs = (N, K) if transb else (K, N)
    A, A1 = binade(rng, (M, K)), binade(rng, (M, K))
    B, B1 = (binade(rng, bs) / np.float32(np.sqrt(K))).astype(np.float32), (binade(rng, bs) / np.float32(np.sqrt(K))).astype(np.float32)
    bias, bias1 = rng.standard_normal(N).astype(np.float32), rng.standard_normal(N).astype(np.float32)
    prev = binade(rng, (M, N), -3, 4)
    return _frozen(A, B, bias, prev, A1, B1, bias1)


def stat_ref(Cgot, rb):
    """[column / 64][row block][sum 64 | sum of squares 64] of the fp32 rows Cgot, in fp64, and the sums of magnitudes (rb rows per block)"""
    M, N = Cgot.shape
    nby, nch = -(-M // rb), -(-N // 64)
    ref, mag = np.zeros((nch, nby, 128)), np.zeros((nch, nby, 128))
    for ch in range(nch):
        for by in range(nby):
            blk = f64(Cgot[by * rb:(by + 1) * rb, ch * 64:(ch + 1) * 64])
            w = blk.shape[1]
            ref[ch, by, :w], ref[ch, by, 64:64 + w] = blk.sum(0), (blk * blk).sum(0)
            mag[ch, by, :w], mag[ch, by, 64:64 + w] = np.abs(blk).sum(0), (blk * blk).sum(0)
    return ref.reshape(1, -1), mag.reshape(1, -1)


# The activation cases take A / 8 (a power of two: the same planes, the same rounding).  A sigmoid's or tanh's error relative to the tensor is the
# pre-activation's ABSOLUTE error, and with thirteen binades |A| |B| reaches a hundred times the activation's range: 2e-6 of that is the 1e-4 bar itself
# (measured with A unscaled: 8.3e-5 on tanh behind a six-product K = 96 product).  An eighth of the magnitude leaves the bar to faults, not to fp32.
EPI_SCALE = np.float32(0.125)


def gemm_go_refuses(M, N, K, mode=0, bias=False, act=0, accumulate=0, stat=False, addg=False):
    """gemm.hip gemm_go's conditions"""
    return bool(M <= 0 or N <= 0 or K <= 0 or (mode == 2 and K % 32) or (stat and (bias or act or accumulate or mode)) or addg)


# (name, arguments of gemm_go_refuses): every one is refused; shared with the GPU test, which makes the call
F32_REFUSALS = (
    ("stat_part with bias", dict(M=130, N=128, K=33, stat=True, bias=True)),
    ("stat_part with act", dict(M=130, N=128, K=33, stat=True, act=3)),
    ("stat_part with accumulate", dict(M=130, N=128, K=33, stat=True, accumulate=1)),
    ("addg", dict(M=130, N=128, K=33, addg=True)),
    ("addg with stat_part", dict(M=130, N=128, K=33, stat=True, addg=True)),
    ("mode 2, K = 48", dict(M=65, N=63, K=48, mode=2)),
    ("stat_part with mode 2", dict(M=65, N=63, K=32, mode=2, stat=True)),      # the launchers of modes 1..4 take no epilogue: the entry point refuses
    ("M = 0", dict(M=0, N=63, K=32)),
)


# ---------------------------------------------------------------- gemm_sb_kernel / gemm_sb16_kernel
SB_MS = (1, 31, 32, 33, 127, 128, 129, 257)
FORM4, FORM16 = 4, 8                      # gsb_dbg bit 2: the 4-wave kernel, bit 3: the 16-wave kernel
GENERIC16, GENERIC4 = 16, 32              # gsb_dbg bit 4 / bit 5: the runtime loop of the 16-wave / the 4-wave kernel where an unrolled instance exists
# (K, mode): the 16-wave kernel's instance is NG = K / 32 (x 2 in mode 2) where listed in launch_gemm_sb, else the runtime loop; the 4-wave kernel
# has NG = 4 at K = 128 (modes 0, 1)
SB_KS = ((32, 0), (96, 0), (160, 0), (128, 0), (256, 0), (384, 0), (512, 0), (384, 2), (1152, 0))
SB_UNROLLED16 = {(128, 0): 4, (256, 0): 8, (384, 0): 12, (512, 0): 16, (384, 2): 24, (1152, 0): 36}
SB_VARIANTS = ("fwd", "bwd4", "bwd6")     # forward (six products), backward under bwd_four_products 1 and 0
CONV_IMAGES = ((2, 3, 2), (1, 1, 1), (3, 1, 5))
SB_CONV = tuple((C, img) for C in (32, 128) for img in CONV_IMAGES) + ((256, (1, 2, 2)),)      # C = 256: the NG = 72 instance


@functools.lru_cache(maxsize=None)
def sb_inputs(M, N, K, transb, seed=16):
    """A0, A1 [M, K]; B0, B1 ([K, N], transb: [N, K]); bias0, bias1; the C before an accumulate; addg [M, N]"""
    rng = np.random.default_rng([seed, M, N, K, transb])
    bs = (N, K) if transb else (K, N)
    A0, A1 = binade(rng, (M, K)), binade(rng, (M, K))
    B0, B1 = ((binade(rng, bs) / np.float32(np.sqrt(K))).astype(np.float32) for _ in range(2))
    b0, b1 = rng.standard_normal(N).astype(np.float32), rng.standard_normal(N).astype(np.float32)
    prev, addg = binade(rng, (M, N), -3, 4), binade(rng, (M, N), -3, 4)
    return _frozen(A0, A1, B0, B1, b0, b1, prev, addg)


def gates(M, ldc, seed=5, all_off=False):
    """gate4 for an [M][ldc] tensor: bit (e & 3) of byte e >> 2, e = row * ldc + column; and the 0 / 1 array [M, ldc] it means"""
    nbytes = (M * ldc + 3) // 4
    g = np.zeros(nbytes, np.uint8) if all_off else np.random.default_rng([seed, M, ldc]).integers(0, 256, nbytes, dtype=np.uint8)
    e = np.arange(M * ldc)
    on = ((g[e >> 2] >> (e & 3)) & 1).reshape(M, ldc)
    return _frozen(g, on)


@functools.lru_cache(maxsize=None)
def conv_inputs(C, img, N=128, seed=9):
    """x [B, H, W, C], w HWIO [3, 3, C, N], dz [B, H, W, N]"""
    B, H, W = img
    rng = np.random.default_rng([seed, C, B, H, W, N])
    x = binade(rng, (B, H, W, C), -4, 5)
    w = (binade(rng, (3, 3, C, N), -4, 5) / np.float32(np.sqrt(9 * C))).astype(np.float32)
    dz = binade(rng, (B, H, W, N), -4, 5)
    return _frozen(x, w, dz)


def im2col3x3(x):
    """[B, H, W, C] -> [B H W, 9 C]: column (tap, c) of pixel (b, t, f) is x[b, t + tap // 3 - 1, f + tap % 3 - 1, c], zero outside the image"""
    B, H, W, C = x.shape
    xp = np.zeros((B, H + 2, W + 2, C), x.dtype)
    xp[:, 1:-1, 1:-1] = x
    cols = [xp[:, dy:dy + H, dx:dx + W].reshape(B * H * W, C) for dy in range(3) for dx in range(3)]
    return np.concatenate(cols, axis=1)


def conv_fwd_ref(x, w):
    """fp64 conv2d (3 x 3 'same', NHWC / HWIO) and the magnitude denominator"""
    import torch
    import torch.nn.functional as F

    def go(a, b):
        return F.conv2d(torch.as_tensor(f64(a)).permute(0, 3, 1, 2), torch.as_tensor(f64(b)).permute(3, 2, 0, 1), padding=1).permute(0, 2, 3, 1).numpy()
    N = w.shape[3]
    return go(x, w).reshape(-1, N), go(np.abs(x), np.abs(w)).reshape(-1, N)


def conv_grads_ref(x, w, dz):
    """fp64 gradients of conv2d w.r.t. the image [B H W, C] and the kernel [9 C, N], by autograd"""
    import torch
    import torch.nn.functional as F
    xt = torch.as_tensor(f64(x)).requires_grad_()
    wt = torch.as_tensor(f64(w)).requires_grad_()
    y = F.conv2d(xt.permute(0, 3, 1, 2), wt.permute(3, 2, 0, 1), padding=1).permute(0, 2, 3, 1)
    dx, dw = torch.autograd.grad(y, (xt, wt), torch.as_tensor(f64(dz)))
    return dx.numpy().reshape(-1, x.shape[3]), dw.numpy().reshape(-1, w.shape[3])


def dgrad_matrix(w):
    """the [9 N, C] matrix of the input-gradient convolution of w HWIO [3, 3, C, N]: row (tap', n) = w[8 - tap', :, n] (prep.h, transb == 2)"""
    C, N = w.shape[2], w.shape[3]
    return np.ascontiguousarray(w.reshape(9, C, N)[::-1].transpose(0, 2, 1).reshape(9 * N, C))


def gemm_sb_refuses(M, N, K, lda=None, ldc=None, mode=0, a0_off=0, a1_off=0, bias=False, act=0, accum=0, stat=False, addg=False, gate=True, conv_C=0,
                    H=0, W=0):
    """gemm_sb.hip launch_gemm_sb's conditions (a*_off: floats the base pointer is off 16-byte alignment)"""
    lda = K if lda is None else lda
    ldc = N if ldc is None else ldc
    if conv_C:
        if conv_C & (conv_C - 1) or conv_C < 32 or K != 9 * conv_C or mode or H <= 0 or W <= 0 or M % (H * W):
            return True
        lda = conv_C

    def usable(off):
        return K % 32 == 0 and N % 128 == 0 and lda % 4 == 0 and off % 4 == 0
    if M <= 0 or N <= 0 or K <= 0 or not usable(a0_off) or (mode == 2 and not usable(a1_off)):
        return True
    if stat and (bias or act or mode or accum):
        return True
    return bool(addg and (not gate or ldc % 4 or mode))


SB_REFUSALS = (
    ("mode 2, A1 off alignment", dict(M=33, N=128, K=96, mode=2, a1_off=1)),
    ("stat_part with bias", dict(M=33, N=128, K=96, stat=True, bias=True)),
    ("conv_C = 48", dict(M=12, N=128, K=432, conv_C=48, H=3, W=2)),
    ("M % (H W) != 0", dict(M=13, N=128, K=288, conv_C=32, H=3, W=2)),
    ("addg with ldc = N + 1", dict(M=33, N=128, K=96, ldc=129, addg=True)),
    ("addg without gate4", dict(M=33, N=128, K=96, addg=True, gate=False)),
    ("N = 100", dict(M=33, N=100, K=96)),
)


# ---------------------------------------------------------------- gemm_tn_kernel
TnCase = namedtuple("TnCase", "M K1 N chunk max_splits pad S shift nslab")
# nslab: what launch_gemm_tn's rule gives (160-row splits, capped, rounded up to whole chunks); pad: 0 tight, 4 lda / ldb + 4, 1 + 1, -1 bases off by one float
TN_CASES = (
    TnCase(1, 1, 129, 32, 0, 0, 0, 0, 1), TnCase(31, 63, 1, 32, 0, 4, 0, 0, 1), TnCase(32, 64, 64, 32, 0, 0, 0, 0, 1),
    TnCase(33, 65, 63, 32, 0, 1, 0, 0, 1), TnCase(160, 129, 65, 32, 0, -1, 0, 0, 1), TnCase(161, 64, 129, 32, 0, 4, 0, 0, 2),
    TnCase(321, 63, 64, 32, 0, 0, 0, 0, 3),
    TnCase(65, 64, 65, 64, 0, 0, 0, 0, 1), TnCase(129, 65, 64, 64, 0, 4, 0, 0, 1), TnCase(321, 129, 63, 64, 0, 1, 0, 0, 3),
    TnCase(321, 65, 65, 32, 1, 0, 0, 0, 1), TnCase(641, 64, 63, 32, 3, 4, 0, 0, 3),
    TnCase(641, 1, 65, 32, 0, 0, 0, 0, 5),       # five splits of 160 rows, the last a single row (M = 161 takes two of 96: its second has 65 rows)
    # shifts: S = 1 masks every row; 320 = 64 x 5 splits at row 160, a sequence boundary; 322 = 46 x 7 splits at rows 128 and 256, inside sequences,
    # and sequence boundaries fall inside every 32-row chunk
    TnCase(33, 65, 63, 32, 0, 0, 1, 1, 1), TnCase(33, 65, 63, 32, 0, 0, 1, -1, 1),
    TnCase(320, 64, 65, 32, 0, 0, 5, 1, 2), TnCase(320, 64, 65, 32, 0, 4, 5, -1, 2),
    TnCase(322, 63, 64, 32, 0, 1, 7, 1, 3), TnCase(322, 63, 64, 64, 0, 0, 7, -1, 3),
)


def tn_id(c):
    return f"M{c.M}-K{c.K1}-N{c.N}-cr{c.chunk}-ms{c.max_splits}-pad{c.pad}-S{c.S}-sh{c.shift}"


def tn_splits(M, max_splits=0, chunk=32):
    """launch_gemm_tn's split rule"""
    splits = min((M + 159) // 160, max_splits if max_splits > 0 else 128)
    rps = -(-M // splits)
    rps = -(-rps // chunk) * chunk
    return -(-M // rps)


@functools.lru_cache(maxsize=None)
def tn_inputs(M, K1, N, seed=6):
    """A [M, K1], B [M, N]"""
    rng = np.random.default_rng([seed, M, K1, N])
    return _frozen(binade(rng, (M, K1), -5, 6), binade(rng, (M, N), -5, 6))


def shifted(A, M, S, shift):
    """rows of A moved by `shift` inside each S-row sequence, zero where the source row lies outside it"""
    out = np.zeros((M, A.shape[1]), A.dtype)
    if shift == 0:
        out[:] = A[:M]
        return out
    for m in range(M):
        if 0 <= m % S + shift < S:
            out[m] = A[m + shift]
    return out


def tn_ref(A, B, M, S=0, shift=0):
    """(C fp64, its magnitude, colsum fp64, its magnitude)"""
    As = shifted(A, M, S if S > 0 else M, shift)
    return f64(As).T @ f64(B), np.abs(f64(As)).T @ np.abs(f64(B)), f64(B).sum(0), np.abs(f64(B)).sum(0)


# ---------------------------------------------------------------- gemm_tn_sb_kernel
TNSB_MS = (1, 31, 33, 160, 161)
TNSB_S = 5
TNSB_JOBS = ((0, 0), (-1, 4), (1, 8), (0, 132))      # per job: (shift, lda - 128)
TNSB_FORMS = ("six", "four", "one")
TNSB_TILES = tuple((K1, N, M) for K1 in (256, 384) for N in (128, 256) for M in (129, 300))
TNSB_CONV = tuple((128, img) for img in CONV_IMAGES) + ((256, (1, 2, 2)),)


def whole_sequences(M, S):
    return -(-M // S) * S


@functools.lru_cache(maxsize=None)
def tnsb_inputs(M, N, job, seed=21):
    rng = np.random.default_rng([seed, M, N, job])
    return _frozen(binade(rng, (whole_sequences(M, TNSB_S), 128), -5, 6), binade(rng, (M, N), -5, 6))


def tn_tile_splits(M, K1, N, slab_cap, tn_tile_blocks=384):
    """launch_gemm_tn_sb_tiles's split rule"""
    tiles = (K1 // 128) * (N // 128)
    splits = min(-(-tn_tile_blocks // tiles), slab_cap // (K1 * N), 128, (M + 127) // 128)
    rps = -(-(-(-M // splits)) // 32) * 32
    return -(-M // rps)


# ---------------------------------------------------------------- reductions
RED_NSLABS = (1, 7, 8, 9, 31, 32, 33, 65)
RED_NS = (1, 31, 32, 33, 100)
RED_2STAGE = (64, 65, 130)


@functools.lru_cache(maxsize=None)
def slabs(nslab, stride, seed=2):
    return _frozen(binade(np.random.default_rng([seed, nslab, stride]), (nslab, stride), -5, 6))


# ---------------------------------------------------------------- heads
HEADS_CASES = ((1, 1, 1, 1), (5, 3, 12, 36), (128, 128, 14, 50), (575, 2, 1, 2))      # (K, Hd, n0, n1)


@functools.lru_cache(maxsize=None)
def heads_inputs(K, Hd, n0, n1, seed=8):
    """per head: w1 [K, Hd], b1 [Hd], w2 [Hd, n], b2 [n]; F [K, n0 + n1], cs [n0 + n1]"""
    rng = np.random.default_rng([seed, K, Hd, n0, n1])
    heads = tuple((binade(rng, (K, Hd), -3, 4), binade(rng, (Hd,), -3, 4), binade(rng, (Hd, n), -3, 4), binade(rng, (n,), -3, 4)) for n in (n0, n1))
    F, cs = binade(rng, (K, n0 + n1), -3, 4), binade(rng, (n0 + n1,), -3, 4)
    for h in heads:
        _frozen(*h)
    return heads, _frozen(F), _frozen(cs)


def heads_weff_ref(heads):
    """the comment above heads_weff_kernel: rows 0..K-1 = [W1s W2s | W1d W2d], row K = [b1s W2s + b2s | b1d W2d + b2d]; and the magnitudes"""
    ref = np.concatenate([np.vstack([f64(w1) @ f64(w2), f64(b1) @ f64(w2) + f64(b2)]) for w1, b1, w2, b2 in heads], axis=1)
    mag = np.concatenate([np.vstack([np.abs(f64(w1)) @ np.abs(f64(w2)), np.abs(f64(b1)) @ np.abs(f64(w2)) + np.abs(f64(b2))]) for w1, b1, w2, b2 in heads], axis=1)
    return ref, mag


def heads_grad_ref(heads, F, cs):
    """per head (dW1, db1, dW2, db2) = (F W2^T, cs W2^T, W1^T F + b1 (x) cs, cs) on the head's columns, each with its magnitude"""
    out, c0 = [], 0
    for w1, b1, w2, b2 in heads:
        n = w2.shape[1]
        Fh, ch = f64(F[:, c0:c0 + n]), f64(cs[c0:c0 + n])
        a = np.abs
        out.append(((Fh @ f64(w2).T, a(Fh) @ a(f64(w2)).T), (ch @ f64(w2).T, a(ch) @ a(f64(w2)).T),
                    (f64(w1).T @ Fh + np.outer(f64(b1), ch), a(f64(w1)).T @ a(Fh) + np.outer(a(f64(b1)), a(ch))), (ch, a(ch))))
        c0 += n
    return out


def heads_refuses(K, n0, n1, prep=False):
    """launch_heads_weff: n0 + n1 > 64; launch_weight_prep also K + 1 > 4 * 144 rows"""
    return n0 + n1 > 64 or (prep and K + 1 > 576)


GSB_MAX_JOBS, TN_MAX_JOBS = 16, 4
PREP_CASES = ((0, 0, True), (2, 1, True), (GSB_MAX_JOBS, 8, False))      # (GEMM split jobs, conv split jobs, folded head weights)
PREP_SHAPES = ((128, 384, 0), (384, 128, 1), (32, 128, 0), (96, 256, 1))       # (K, N, transb) of GEMM split job i % 4
MUL_NS = (4, 1028)


# ---------------------------------------------------------------- the operands of every four-product case
SB_NATURAL = ((256, 0, 128), (256, 0, 96), (128, 1, 128), (128, 1, 96))      # (N, mode, K): what the launcher picks the 4-wave kernel for
SB_CONV_BWD = ((128, (2, 3, 2)), (128, (3, 1, 5)))
TN_TILE_FORMS = ("six", "four")


def four_cases():
    """(name, A, B) with the product f64(A) @ f64(B), for every call the GPU test makes in the four-product form"""
    for M in SB_MS:
        i = sb_inputs(M, 128, 128, 1)
        yield f"sb rows M{M}", i[0], i[2].T
    for K, mode in SB_KS:
        i = sb_inputs(129, 128, K, 1)
        if mode == 2:
            yield f"sb K{K} mode 2", np.hstack([i[0], i[1]]), np.vstack([i[2].T, i[3].T])
        else:
            yield f"sb K{K}", i[0], i[2].T
    for N, mode, K in SB_NATURAL:
        i = sb_inputs(129, N, K, 1)
        yield f"sb N{N} K{K} first", i[0], i[2].T
        if mode == 1:
            yield f"sb N{N} K{K} second", i[0], i[3].T
    for M in (129, 33):
        i = sb_inputs(M, 128, 128, 1)
        yield f"sb addg M{M}", i[0], i[2].T
    for C, img in SB_CONV_BWD:
        x, w, dz = conv_inputs(C, img)
        yield f"sb conv dgrad C{C} {img}", im2col3x3(dz), dgrad_matrix(w)
    for M in TNSB_MS:
        for N in (128, 256):
            for j, (shift, _) in enumerate(TNSB_JOBS):
                A, B = tnsb_inputs(M, N, j)
                yield f"tn_sb M{M} N{N} job{j}", shifted(A, M, TNSB_S, shift).T, B
    for K1, N, M in TNSB_TILES:
        A, B = tn_inputs(M, K1, N)
        yield f"tn_sb tiles K{K1} N{N} M{M}", A.T, B
    for C, img in TNSB_CONV:
        x, w, dz = conv_inputs(C, img)
        yield f"tn_sb conv C{C} {img}", im2col3x3(x).T, dz.reshape(-1, dz.shape[3])
