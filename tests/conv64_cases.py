"""Cases, seeded inputs and plain fp64 references for the 64 -> 64 3x3 convolution family: conv_sb.hip (conv64_fwd_sbd_kernel in its region, FOUR,
ONE, PRE and EXT forms, the generic conv64_fwd_sb_kernel), conv_wgrad_sb.hip (conv64_wgrad_sb_kernel) and the 64 -> 64 kernels of conv.hip
(conv64_fwd_kernel, conv64_wgrad_kernel).  Shared by tests/test_conv64_family_cpu.py (what the cases and bars promise, without a GPU) and
tests/test_conv64_family_gpu.py (the kernels).  Checker only.

Inputs are float32 before anything is computed from them, cached and read-only.  Image, gradient and kernel span nine binades (gemm_cases.binade, a
normal variate times 2^[-4, 4]) so that the mid and lo planes of a split carry weight; the bias is a normal variate, non-zero in every channel: the
out-of-image rows of a partial tile evaluate to partial sums plus the bias, never to zero, so a statistics mask that leaks shows.

Tile geometry, mirrored from the launchers (test_conv64_family_cpu.py reads each value back from seld_amd/csrc):
  form          rows R per tile / chunk                       grid cap   source
  sbd           16 / 48 / 32 at W = 16 / 4 / 8                256        conv_sb.hip conv64_sb: launch_sbd<4, 16>, <2, 48>, <3, 32>; launch_sbd: `ntiles < 256 ? ntiles : 256`
  sbd_four      8 at W = 16                                   512        conv_sb.hip conv64_sb: launch_sbd_four<4, 8>; launch_sbd_four: `ntiles < 512 ? ntiles : 512`
  sb (generic)  256 pixels of the [B H W] axis                512        conv_sb.hip conv64_sb: `(npix + 255) / 256`, SB_MAX_PERSISTENT
  f32           128 pixels of the [B H W] axis                768        conv.hip launch_conv64_fwd: `(npix + 127) / 128`, CONV_MAX_PERSISTENT
  wgrad_sb      64 / W rows (WGSB_PXC pixels)                 512, 256 at W = 4   conv_wgrad_sb.hip launch_conv64_wgrad_sb: WGSB_MAX_BLOCKS, `W == 4 ? WGSB_MAX_BLOCKS / 2`
  wgrad_f32     128 / W rows at W = 16, 96 / W elsewhere      512        conv.hip conv64_wgrad_chunk_px, WGRAD_MAX_BLOCKS
For the two kernels that tile the pixel axis, "R" in the edge table is the number of image rows one tile holds (256 / W, 128 / W).

Edge table (EDGE_HS): B = 3 — the middle clip has a neighbour on both sides — and H in {1, 2, R - 1, R, R + 1, 2 R + 1}.

Over-cap table (OVER): per launcher the shape B = cap + 2, H = R + 1: two tiles per image, the second of one row, 2 cap + 4 tiles — more than twice
the cap and no multiple of it: workgroups 0 .. 3 run three tiles, the others two, and the third round holds two full tiles and two one-row tiles.
The pixel-axis kernels take B = 3 and the smallest H that gives 2 cap + 1 tiles (clip boundaries then fall inside tiles, the last tile holds 32, 2
or 48 pixels); at W = 32 conv64_fwd_kernel runs the generic kernel's shape, 2049 = 2 x 768 + 513 of its 128-pixel tiles, so that one reference
serves both.
Tile counts (test_over_cap_tile_counts recomputes them from R and the cap):
  sbd W16 (258, 17): 516      sbd W4 (258, 49): 516       sbd W8 (258, 33): 516      sbd_four W16 (514, 9): 1028
  sb W32 (3, 2731): 1025      sb W2 (3, 43691): 1025      f32 W16 (3, 4097): 1537    f32 W32 (3, 2731): 2049
  wgrad_sb W16 (514, 5): 1028     W8 (514, 9): 1028     W4 (258, 17): 516 (the halved cap)     wgrad_f32 W16 (514, 9): 1028

Bars (all from the project):
  helpers.check, 1e-4 tensor-normalised: every tensor.
  BAR6 = BAR1 = 2e-6 (gemm_cases.py) on |got - ref| / (conv of |x| with |w|, plus |bias|): the six-product kernels, the fp32 kernels, and the
      single-product kernels against the fp64 result of the bf16-rounded operands.  Statistics meet it against the fp64 sums of the rows the kernel
      itself stored, over sum |v| and sum v^2 (gemm_cases' treatment of stat_part).
  BAR4 = FOUR_EMUL + 2e-6: the four-product forms.  FOUR_EMUL is the largest magnitude-normalised error, over the inputs of every four-product call the
      GPU test makes (four_cases()), of the form's exact arithmetic — two planes per operand with the rounded mid of sb_tile.h split2r_pair, the four
      retained products, fp64 accumulation — against the fp64 reference.  test_conv64_family_cpu.py::test_four_product_emulation measures it (the
      [four] lines it prints) and holds it under the constant.
      Measured: 2.594e-5 (kernel gradient, W = 4, (B, H) = (3, 2): sums over 24 pixels, where little averages out); the kernel gradients of the other
      one- and two-row images follow at 1.7e-5 .. 2.3e-5, the over-cap kernel gradients stay below 1e-5; the input gradients (sums of up to 576 terms)
      lie between 7.7e-6 and 1.33e-5, the over-cap shapes highest (the maximum over the most elements).  Two operands of 16 significant bits each, the
      second plane rounded: 2 * 2^-16 = 3.1e-5 at worst.

The float32 evaluation of every case (test_float32_evaluation_is_within_half_the_bars) measured at most 5.1e-7, 0.26 of BAR6, on the CPU (conv32 / wgrad_product in float32:
products over 64 terms, summed pairwise)."""
import functools
from collections import namedtuple

import numpy as np

from gemm_cases import BAR1, BAR6, bf16_rne, binade, f64, mag_err, two_planes_rounded      # noqa: F401
from aux_kernel_cases import report, report_exact      # noqa: F401

FOUR_EMUL = 2.6e-5
BAR4 = FOUR_EMUL + 2e-6
assert BAR4 < 1e-4

C = 64
B_EDGE = 3

# ---------------------------------------------------------------- tile geometry
SBD_R = {16: 16, 4: 48, 8: 32}
SBD_CAP = 256
SBD_FOUR_R, SBD_FOUR_CAP = 8, 512
SB_TILE_PX, SB_CAP = 256, 512
F32_TILE_PX, F32_CAP = 128, 768
WGSB_PXC, WGSB_CAP = 64, 512
WGRAD_CAP = 512
WGRAD_WIDTHS = (16, 8, 4, 32, 2)


def wgsb_cap(W):
    return WGSB_CAP // 2 if W == 4 else WGSB_CAP


def wgrad_chunk_px(W):
    return 128 if W == 16 else 96


Form = namedtuple("Form", "name W R cap px_axis")      # px_axis: tiles are runs of R * W pixels of the [B H W] axis, not rows of one image


def _forms():
    out = {}
    for W, R in SBD_R.items():
        out[f"sbd{W}"] = Form(f"sbd{W}", W, R, SBD_CAP, False)
    out["sbd_four16"] = Form("sbd_four16", 16, SBD_FOUR_R, SBD_FOUR_CAP, False)
    for W in (32, 2):
        out[f"sb{W}"] = Form(f"sb{W}", W, SB_TILE_PX // W, SB_CAP, True)
    for W in (16, 32):
        out[f"f32_{W}"] = Form(f"f32_{W}", W, F32_TILE_PX // W, F32_CAP, True)
    for W in (16, 8, 4):
        out[f"wgsb{W}"] = Form(f"wgsb{W}", W, WGSB_PXC // W, wgsb_cap(W), False)
    for W in WGRAD_WIDTHS:
        out[f"wgf32_{W}"] = Form(f"wgf32_{W}", W, wgrad_chunk_px(W) // W, WGRAD_CAP, False)
    return out


FORMS = _forms()


def edge_hs(R):
    """H of the edge table for tiles of R rows (a set: R = 3 gives R - 1 = 2)"""
    return tuple(sorted({1, 2, R - 1, R, R + 1, 2 * R + 1} - {0}))


EDGE_HS = {name: edge_hs(f.R) for name, f in FORMS.items()}


def ntiles(form, B, H):
    f = FORMS[form]
    if f.px_axis:
        return -(-(B * H * f.W) // (f.R * f.W))
    return B * (-(-H // f.R))


def _over_rows(form):
    f = FORMS[form]
    return (f.cap + 2, f.R + 1)


# form -> (B, H); the tile counts are in the docstring and in OVER_TILES
OVER = {name: _over_rows(name) for name in ("sbd16", "sbd4", "sbd8", "sbd_four16", "wgsb16", "wgsb8", "wgsb4", "wgf32_16")}
OVER["sb32"] = (3, 2731)
OVER["sb2"] = (3, 43691)
OVER["f32_16"] = (3, 4097)
OVER["f32_32"] = (3, 2731)
OVER_TILES = {"sbd16": 516, "sbd4": 516, "sbd8": 516, "sbd_four16": 1028, "sb32": 1025, "sb2": 1025, "f32_16": 1537, "f32_32": 2049, "wgsb16": 1028,
              "wgsb8": 1028, "wgsb4": 516, "wgf32_16": 1028}


def shapes(form, over=True):
    """(B, H) of the edge table, then the over-cap shape where the form's launcher has one"""
    out = [(B_EDGE, H) for H in EDGE_HS[form]]
    if over and form in OVER:
        out.append(OVER[form])
    return tuple(out)


# ---------------------------------------------------------------- inputs
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def weights(seed=64):
    """w HWIO [3, 3, 64, 64], bias [64] (no zero), and the kernel whose input gradient is the convolution with w: wd[tap][ci][co] = w[8 - tap][co][ci]
    (conv.hip flip_weights_kernel is an involution), so conv3x3_dgrad(dz, wd) = conv(dz, w) without bias and one reference serves both"""
    rng = np.random.default_rng(seed)
    w = (binade(rng, (3, 3, C, C), -4, 5) / np.float32(24)).astype(np.float32)
    bias = rng.standard_normal(C).astype(np.float32)
    assert (bias != 0).all()
    wd = np.ascontiguousarray(w.reshape(9, C, C)[::-1].transpose(0, 2, 1)).reshape(3, 3, C, C)
    return _frozen(w, bias, wd)


@functools.lru_cache(maxsize=None)
def images(B, H, W, seed=65):
    """x [B, H, W, 64] (the forward's image, the input gradient's dz, the kernel gradient's image) and dz [B, H, W, 64] (the kernel gradient's)"""
    rng = np.random.default_rng([seed, B, H, W])
    return _frozen(binade(rng, (B, H, W, C), -4, 5), binade(rng, (B, H, W, C), -4, 5))


@functools.lru_cache(maxsize=None)
def pre_params(seed=66):
    """scale, shift [64] of the previous block's BatchNorm (both signs of scale: about half of every channel survives the ReLU), and the gamma of this
    block's: negative entries, an exact 0 and a -0.0; scale2 = gamma * invstd, shift2: what the next block's loader applies to the window extremes"""
    rng = np.random.default_rng(seed)
    scale = (rng.standard_normal(C) * np.exp2(rng.integers(-2, 3, C))).astype(np.float32)
    shift = rng.standard_normal(C).astype(np.float32)
    gamma = rng.standard_normal(C).astype(np.float32)
    gamma[5], gamma[37] = np.float32(0.0), np.float32(-0.0)
    gamma[0], gamma[33] = -abs(gamma[0]), -abs(gamma[33])      # a negative entry in both channel halves, whatever the draw
    assert (gamma < 0).sum() >= 8 and (gamma > 0).sum() >= 8 and np.signbit(gamma[37]) and gamma[37] == 0
    invstd = (np.float32(1) / (np.float32(0.5) + rng.random(C).astype(np.float32))).astype(np.float32)
    scale2 = (gamma * invstd).astype(np.float32)
    shift2 = rng.standard_normal(C).astype(np.float32)
    return _frozen(scale, shift, gamma, scale2, shift2)


def fma32(v, s, t):
    """float32 fmaf(v, s, t), exactly: v * s is exact in float64 (24 + 24 bits); the sum is rounded to ODD in float64 (TwoSum gives the sign of what the
    round-to-nearest sum dropped), and 53 >= 24 + 2 bits round-to-odd followed by round-to-nearest float32 is the correctly rounded float32"""
    p = f64(v) * f64(s)
    t = np.broadcast_to(f64(t), p.shape)
    sm = p + t
    bb = sm - p
    err = (p - (sm - bb)) + (t - bb)                         # TwoSum: p + t = sm + err exactly
    even = (sm.view(np.int64) & 1) == 0
    toward = np.where(err > 0, np.inf, -np.inf)
    odd = np.where((err != 0) & even, np.nextafter(sm, toward), sm)
    return odd.astype(np.float32)


def act32(x, scale, shift):
    """the PRE loader / bn_relu_ext: max(0, fmaf(v, scale[c], shift[c])) in float32"""
    return np.maximum(np.float32(0), fma32(x, scale, shift))


@functools.lru_cache(maxsize=None)
def activated(B, H, W):
    scale, shift = pre_params()[:2]
    return _frozen(act32(images(B, H, W)[0], scale, shift))


def ext_select(z, gamma):
    """per (1, 4) window of bins and channel: the maximum of z where gamma >= 0, the minimum where gamma < 0 (-0.0 and 0 take the maximum); [B, H, W / 4, 64]"""
    B, H, W, _ = z.shape
    zw = z.reshape(B, H, W // 4, 4, C)
    return np.where(np.asarray(gamma) < 0, zw.min(axis=3), zw.max(axis=3))


# ---------------------------------------------------------------- references
def conv64(x, w):
    """fp64 3 x 3 'same' convolution NHWC / HWIO, no bias"""
    import torch
    import torch.nn.functional as F
    return F.conv2d(torch.as_tensor(f64(x)).permute(0, 3, 1, 2), torch.as_tensor(f64(w)).permute(3, 2, 0, 1), padding=1).permute(0, 2, 3, 1).contiguous().numpy()


def tree_sum(parts):
    """pairwise sum of a list of equal arrays, in their dtype"""
    parts = list(parts)
    while len(parts) > 1:
        parts = [parts[i] + parts[i + 1] if i + 1 < len(parts) else parts[i] for i in range(0, len(parts), 2)]
    return parts[0]


def conv32(x, w, bias=None):
    """the same in float32, in the kernels' own hierarchy: one tap is a float32 product over its 64 channels, the nine taps are summed pairwise"""
    x, w = np.asarray(x, np.float32), np.asarray(w, np.float32)
    out = tree_sum([_shift(x, tap // 3, tap % 3) @ w[tap // 3, tap % 3] for tap in range(9)]).reshape(x.shape)
    return out if bias is None else out + np.asarray(bias, np.float32)


def _operand(kind, B, H, W):
    x = images(B, H, W)[0]
    if kind == "act":
        return activated(B, H, W)
    return x


@functools.lru_cache(maxsize=None)
def fwd_ref(kind, B, H, W):
    """(conv(x, w) in fp64 without bias, conv(|x|, |w|)) for kind "x" (the image), "one" (image and kernel rounded to bf16: single-product mode) and
    "act" (the activated image of the PRE chain).  Forward adds the bias to both (with_bias); the input gradient of weights()[2] is the first as it is"""
    w = weights()[0]
    x = _operand(kind, B, H, W)
    if kind == "one":
        x, w = bf16_rne(x), bf16_rne(w)
    return _frozen(conv64(x, w), conv64(np.abs(x), np.abs(w)))


def with_bias(ref, mag):
    bias = f64(weights()[1])
    return ref + bias, mag + np.abs(bias)


def dgrad_autograd(dz, wd):
    """the input gradient by autograd, fp64 (the small shapes: it shows that fwd_ref serves the input gradient of weights()[2])"""
    import torch
    import torch.nn.functional as F
    x = torch.zeros(dz.shape, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x.permute(0, 3, 1, 2), torch.as_tensor(f64(wd)).permute(3, 2, 0, 1), padding=1).permute(0, 2, 3, 1)
    (g,) = torch.autograd.grad(y, x, torch.as_tensor(f64(dz)))
    return g.numpy()


def _shift(x, dy, dx):
    """x[b, t + dy - 1, f + dx - 1], zero outside the image, as [B H W, 64]"""
    B, H, W, _ = x.shape
    xp = np.zeros((B, H + 2, W + 2, C), x.dtype)
    xp[:, 1:-1, 1:-1] = x
    return xp[:, dy:dy + H, dx:dx + W].reshape(-1, C)


def wgrad_product(x, dz, dtype=np.float64):
    """dW[tap][ci][co] = sum over pixels of x[pixel + tap][ci] dz[pixel][co] -> [9, 64, 64]; db[co] = sum dz.  In float32: products over blocks of 64
    pixels (a chunk of conv64_wgrad_sb_kernel), the blocks summed pairwise"""
    x, dz = np.asarray(x, dtype), np.asarray(dz, dtype).reshape(-1, C)
    if dtype == np.float64:
        return np.stack([_shift(x, tap // 3, tap % 3).T @ dz for tap in range(9)]), dz.sum(0)
    n = dz.shape[0]
    nb = -(-n // 64)

    def blocks(a):
        out = np.zeros((nb * 64, C), dtype)
        out[:n] = a
        return out.reshape(nb, 64, C)
    db = blocks(dz)
    dw = np.stack([tree_sum(list(np.matmul(blocks(_shift(x, tap // 3, tap % 3)).transpose(0, 2, 1), db))) for tap in range(9)])
    return dw, tree_sum(list(db.reshape(-1, C)))


@functools.lru_cache(maxsize=None)
def wgrad_ref(kind, B, H, W):
    """(dW fp64 [9, 64, 64], its magnitude, db fp64 [64], its magnitude); kind "x" or "one" (both operands rounded to bf16; db sums the unrounded dz)"""
    x, dz = images(B, H, W)
    xs, ds = (bf16_rne(x), bf16_rne(dz)) if kind == "one" else (x, dz)
    dw, _ = wgrad_product(xs, ds)
    mw, _ = wgrad_product(np.abs(xs), np.abs(ds))
    return _frozen(dw, mw, f64(dz).reshape(-1, C).sum(0), np.abs(f64(dz)).reshape(-1, C).sum(0))


def stats_ref(zgot):
    """[sum 64 | sum of squares 64] of the stored rows in fp64, and the sums of magnitudes"""
    v = f64(zgot).reshape(-1, C)
    return np.concatenate([v.sum(0), (v * v).sum(0)]), np.concatenate([np.abs(v).sum(0), (v * v).sum(0)])


def four_emulation(kind, B, H, W):
    """the four-product form's exact arithmetic: both operands on two planes (rounded mid), the product in fp64; (hi + mid)(hi' + mid') is the four
    retained products.  kind "dgrad": conv(x, w); "wgrad": the kernel gradient of (x, dz)"""
    x, dz = images(B, H, W)
    if kind == "dgrad":
        return conv64(two_planes_rounded(x), two_planes_rounded(weights()[0]))
    return wgrad_product(two_planes_rounded(x), two_planes_rounded(dz))[0]


# ---------------------------------------------------------------- the forms the GPU test runs
# forward: (id, tile form, options, reference kind, bar)
FWD_FORMS = (
    ("six-W16", "sbd16", {}, "x", BAR6), ("six-W8", "sbd8", {}, "x", BAR6), ("six-W4", "sbd4", {}, "x", BAR6),
    ("one-W16", "sbd16", {"bf16_single": 1}, "one", BAR1), ("one-W4", "sbd4", {"bf16_single": 1}, "one", BAR1),
    ("generic-W32", "sb32", {}, "x", BAR6), ("generic-W2", "sb2", {}, "x", BAR6),
    ("f32-W16", "f32_16", {"conv64_split_bf16": 0}, "x", BAR6), ("f32-W32", "f32_32", {"conv64_split_bf16": 0}, "x", BAR6),
)
# input gradient
DGRAD_FORMS = (
    ("six-W16", "sbd16", {"bwd_four_products": 0}, "x", BAR6), ("six-W8", "sbd8", {"bwd_four_products": 0}, "x", BAR6),
    ("six-W4", "sbd4", {"bwd_four_products": 0}, "x", BAR6), ("six-W32", "sb32", {"bwd_four_products": 0}, "x", BAR6),
    ("six-W2", "sb2", {"bwd_four_products": 0}, "x", BAR6),
    ("four-R16-W16", "sbd16", {"dgrad_r8": 0}, "x", BAR4), ("four-R8-W16", "sbd_four16", {"dgrad_r8": 1}, "x", BAR4),
    ("four-W4", "sbd4", {}, "x", BAR4), ("four-W8", "sbd8", {}, "x", BAR4),
    ("one-W16", "sbd16", {"bf16_single": 1}, "one", BAR1),
    ("f32-W16", "f32_16", {"conv64_split_bf16": 0}, "x", BAR6), ("f32-W32", "f32_32", {"conv64_split_bf16": 0}, "x", BAR6),
)
# kernel and bias gradient
WGRAD_FORMS = tuple((f"{name}-W{W}", f"wgsb{W}", opts, kind, bar) for W in (16, 8, 4) for name, opts, kind, bar in (
    ("six", {"bwd_four_products": 0}, "x", BAR6), ("four", {"bwd_four_products": 1}, "x", BAR4), ("one", {"bf16_single": 1}, "one", BAR1))) + tuple(
    (f"f32-W{W}", f"wgf32_{W}", {"conv64_split_bf16": 0}, "x", BAR6) for W in WGRAD_WIDTHS)
PRE_WIDTHS = (16, 4)
DEFAULTS = {"conv64_split_bf16": 1, "bwd_four_products": 1, "bf16_single": 0, "dgrad_r8": 1}


def cases(forms):
    """(form id, B, H) for a parametrised test"""
    return [(f[0], B, H) for f in forms for B, H in shapes(f[1])]


def form_of(forms, fid):
    return next(f for f in forms if f[0] == fid)


def four_cases():
    """(name, kind, B, H, W) of every four-product call of the GPU test"""
    for fid, tf, _, _, bar in DGRAD_FORMS:
        if bar == BAR4:
            for B, H in shapes(tf):
                yield f"dgrad {fid} {B, H}", "dgrad", B, H, FORMS[tf].W
    for fid, tf, _, _, bar in WGRAD_FORMS:
        if bar == BAR4:
            for B, H in shapes(tf):
                yield f"wgrad {fid} {B, H}", "wgrad", B, H, FORMS[tf].W


# ---------------------------------------------------------------- refusals of seld_k_conv3x3_fwd_pre
def fwd_pre_refuses(W, pre=True, pre_shift=True, ext=False, ext_gamma=True, pre_out_is_x=False, single=False):
    """conv_sb.hip: conv64_sb (`(pre_scale || ext_out) && !conv64_fwd_sb_takes_pre`, takes_pre = (W == 16 || W == 4) && !mfma_one) and launch_sbd
    (`kc.mfma_one || !pre_shift || pre_out == x`; `ext_out && !ext_gamma`; W = 4: `if (ext_out) return -3`; without pre_scale: `if (ext_out) return -3`)"""
    takes_pre = W in (16, 4) and not single
    if (pre or ext) and not takes_pre:
        return True
    if pre:
        if single or not pre_shift or pre_out_is_x:
            return True
        if W == 16:
            return bool(ext and not ext_gamma)
        return bool(ext)
    return bool(ext)


PRE_REFUSALS = (
    ("PRE at W = 8", dict(W=8)),
    ("PRE at W = 32", dict(W=32)),
    ("EXT at W = 4", dict(W=4, ext=True)),
    ("EXT without PRE", dict(W=16, pre=False, ext=True)),
    ("EXT without ext_gamma", dict(W=16, ext=True, ext_gamma=False)),
    ("pre_out == x", dict(W=16, pre_out_is_x=True)),
    ("PRE under bf16_single", dict(W=16, single=True)),
)
