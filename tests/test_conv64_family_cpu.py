"""What tests/conv64_cases.py promises, checked without a GPU: the edge and over-cap tables follow from the tile geometry, the geometry is the launchers'
(read from seld_amd/csrc), a float32 evaluation of every case stays within half of its bar, the four-product emulation stays under its constant, the
refusals follow from the launcher's conditions, and what is exact by construction (the activation, the window selection) is exact."""
import math
import os
import re
from fractions import Fraction

import numpy as np

import conv64_cases as K
from conftest import ROOT
from gemm_cases import mag_err

CSRC = os.path.join(ROOT, "seld_amd", "csrc")


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def _define(text, name):
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))


def test_geometry_is_the_launchers():
    sb, wg, cv = _src("conv_sb.hip"), _src("conv_wgrad_sb.hip"), _src("conv.hip")
    # conv64_sb: which region launcher a width takes, and on how many rows
    sbd = {int(w): (int(l), int(r)) for w, l, r in re.findall(r"if \(W == (\d+)\) return launch_sbd<(\d+), (\d+)>\(", sb)}
    assert sbd == {W: (int(math.log2(W)), R) for W, R in K.SBD_R.items()}
    assert re.search(r"if \(W == 16 && four && kc\.dgrad_r8 .*\n\s*return launch_sbd_four<4, (\d+)>\(", sb).group(1) == str(K.SBD_FOUR_R)
    body = sb[sb.index("static int launch_sbd("):sb.index("static int launch_sbd_four(")]
    assert re.search(r"const int grid = ntiles < (\d+) \? ntiles : \1;", body).group(1) == str(K.SBD_CAP)
    body = sb[sb.index("static int launch_sbd_four("):sb.index("int conv64_fwd_sb_takes_pre")]
    assert re.search(r"const int grid = ntiles < (\d+) \? ntiles : \1;", body).group(1) == str(K.SBD_FOUR_CAP)
    assert "const int ntiles = (npix + 255) / 256;" in sb and K.SB_TILE_PX == 256
    assert "ntiles < SB_MAX_PERSISTENT ? ntiles : SB_MAX_PERSISTENT" in sb and _define(sb, "SB_MAX_PERSISTENT") == K.SB_CAP
    assert "const int ntiles = (npix + 127) / 128;" in cv and K.F32_TILE_PX == 128
    assert "ntiles < CONV_MAX_PERSISTENT ? ntiles : CONV_MAX_PERSISTENT" in cv and _define(cv, "CONV_MAX_PERSISTENT") == K.F32_CAP
    assert _define(wg, "WGSB_PXC") == K.WGSB_PXC and _define(wg, "WGSB_MAX_BLOCKS") == K.WGSB_CAP
    assert "const int cap_ = W == 4 ? WGSB_MAX_BLOCKS / 2 : WGSB_MAX_BLOCKS;" in wg and K.wgsb_cap(4) == 256 and K.wgsb_cap(16) == K.wgsb_cap(8) == 512
    assert "int conv64_wgrad_sb_usable(int W) { return W == 16 || W == 8 || W == 4; }" in wg
    a, b = re.search(r"constexpr int conv64_wgrad_chunk_px\(int W\) \{ return W == 16 \? (\d+) : (\d+); \}", cv).groups()
    assert (K.wgrad_chunk_px(16), K.wgrad_chunk_px(8), K.wgrad_chunk_px(32)) == (int(a), int(b), int(b))
    assert _define(cv, "WGRAD_MAX_BLOCKS") == K.WGRAD_CAP
    assert sorted(int(w) for w in re.findall(r"if \(W == (\d+)\) wl = \d;", cv)) == sorted(K.WGRAD_WIDTHS)
    # the rows of a form follow from these
    assert [K.FORMS[f"sbd{W}"].R for W in (16, 4, 8)] == [16, 48, 32] and K.FORMS["sbd_four16"].R == 8
    assert (K.FORMS["sb32"].R, K.FORMS["sb2"].R, K.FORMS["f32_16"].R, K.FORMS["f32_32"].R) == (8, 128, 8, 4)
    assert [K.FORMS[f"wgsb{W}"].R for W in (16, 8, 4)] == [4, 8, 16]
    assert [K.FORMS[f"wgf32_{W}"].R for W in (16, 8, 4, 32, 2)] == [8, 12, 24, 3, 48]


def test_edge_table_holds_every_pair():
    for name, f in K.FORMS.items():
        hs = K.EDGE_HS[name]
        for H in (1, 2, f.R - 1, f.R, f.R + 1, 2 * f.R + 1):
            assert H in hs, (name, H)
        assert all(H >= 1 for H in hs)
    for forms in (K.FWD_FORMS, K.DGRAD_FORMS, K.WGRAD_FORMS):
        listed = set(K.cases(forms))
        for fid, tf, *_ in forms:
            for H in K.EDGE_HS[tf]:
                assert (fid, K.B_EDGE, H) in listed
            if tf in K.OVER:
                assert (fid,) + K.OVER[tf] in listed


def test_over_cap_tile_counts():
    assert set(K.OVER) == set(K.OVER_TILES)
    for name, (B, H) in K.OVER.items():
        f = K.FORMS[name]
        n = K.ntiles(name, B, H)
        assert n == K.OVER_TILES[name], (name, n)
        assert n > 2 * f.cap and n % f.cap != 0 and n < 3 * f.cap      # some workgroups run three tiles, the others two; the last round is partial
        if f.px_axis:
            assert (B * H * f.W) % (f.R * f.W) != 0                     # the last tile is partial
            assert K.ntiles(name, B, H - 1) <= 2 * f.cap or name == "f32_32"      # the smallest H at this B (f32_32 borrows sb32's shape)
        else:
            assert H % f.R == 1 and -(-H // f.R) == 2                   # every image ends in a one-row tile
            assert (B, H) == (f.cap + 2, f.R + 1)
    assert K.OVER["sbd16"] == (258, 17) and K.OVER["sbd4"] == (258, 49)
    # launch_sbd_four is reached by the input gradient alone; the fp32 kernel gradient shares its shape
    assert K.OVER["sbd_four16"] == K.OVER["wgf32_16"] == (514, 9)


def test_inputs_are_float32_frozen_and_spread():
    w, bias, wd = K.weights()
    x, dz = K.images(3, 17, 16)
    for a in (w, bias, wd, x, dz) + K.pre_params():
        assert a.dtype == np.float32 and not a.flags.writeable
    assert (bias != 0).all()
    for a in (w, x, dz):
        e = np.floor(np.log2(np.abs(a[a != 0])))
        assert e.max() - e.min() >= 9          # nine binades of scale under the normal variate
    assert K.images(3, 17, 16)[0] is x
    gamma = K.pre_params()[2]
    assert (gamma < 0).any() and gamma[5] == 0 and not np.signbit(gamma[5]) and gamma[37] == 0 and np.signbit(gamma[37])


def test_input_gradient_is_the_forward_reference():
    """conv3x3_dgrad(dz, weights()[2]) by autograd = conv(dz, weights()[0]): fwd_ref serves both"""
    wd = K.weights()[2]
    for B, H, W in ((3, 2, 16), (3, 9, 4), (2, 3, 32), (3, 5, 2)):
        x = K.images(B, H, W)[0]
        ref, mag = K.fwd_ref("x", B, H, W)
        assert mag_err(K.dgrad_autograd(x, wd), ref, mag) < 1e-14


def _all_cases(forms):
    seen = set()
    for fid, tf, _, kind, bar in forms:
        for B, H in K.shapes(tf):
            key = (kind, B, H, K.FORMS[tf].W)
            if key not in seen:
                seen.add(key)
                yield key


def test_float32_evaluation_is_within_half_the_bars():
    """plain float32 numpy (conv64_cases.conv32, wgrad_product) against the fp64 references, magnitude-normalised: the bars leave room for fp32 itself"""
    w, bias, _ = K.weights()
    worst = 0.0
    for kind, B, H, W in sorted(set(_all_cases(K.FWD_FORMS)) | set(_all_cases(K.DGRAD_FORMS)) | {("act", B, H, W_) for W_ in K.PRE_WIDTHS
                                                                                               for B, H in K.shapes(f"sbd{W_}")}):
        x = K.activated(B, H, W) if kind == "act" else K.images(B, H, W)[0]
        xs, ws = (K.bf16_rne(x).astype(np.float32), K.bf16_rne(w).astype(np.float32)) if kind == "one" else (x, w)
        ref, mag = K.with_bias(*K.fwd_ref(kind, B, H, W))
        got = K.conv32(xs, ws, bias)
        e = mag_err(got, ref, mag)
        worst = max(worst, e)
        assert e <= K.BAR6 / 2, (kind, B, H, W, e)
        sref, smag = K.stats_ref(got)
        v = np.ascontiguousarray(got.reshape(-1, 64).T)          # the pixel axis contiguous: numpy then sums it pairwise, as the kernels sum per lane, wave, workgroup
        s32 = np.concatenate([v.sum(1, dtype=np.float32), (v * v).sum(1, dtype=np.float32)])
        assert mag_err(s32, sref, smag) <= K.BAR6 / 2, (kind, B, H, W)
    for kind, B, H, W in sorted(set(_all_cases(K.WGRAD_FORMS))):
        x, dz = K.images(B, H, W)
        xs, ds = (K.bf16_rne(x).astype(np.float32), K.bf16_rne(dz).astype(np.float32)) if kind == "one" else (x, dz)
        dw, mw, db, mb = K.wgrad_ref(kind, B, H, W)
        gw, _ = K.wgrad_product(xs, ds, np.float32)
        gw, gb = K.wgrad_product(xs, dz, np.float32) if kind != "one" else (gw, K.wgrad_product(x, dz, np.float32)[1])
        e = max(mag_err(gw, dw, mw), mag_err(gb, db, mb))
        worst = max(worst, e)
        assert e <= K.BAR6 / 2, ("wgrad", kind, B, H, W, e)
    print(f"[float32] worst magnitude-normalised error {worst:.3e} = {worst / K.BAR6:.2f} of BAR6")


def test_four_product_emulation():
    worst = 0.0
    for name, kind, B, H, W in K.four_cases():
        if kind == "dgrad":
            ref, mag = K.fwd_ref("x", B, H, W)
        else:
            ref, mag = K.wgrad_ref("x", B, H, W)[:2]
        e = mag_err(K.four_emulation(kind, B, H, W), ref, mag)
        print(f"[four] {name:40s} {e:.3e}")
        worst = max(worst, e)
    print(f"[four] worst {worst:.3e}  FOUR_EMUL {K.FOUR_EMUL:.3e}")
    assert worst <= K.FOUR_EMUL
    assert worst >= K.FOUR_EMUL / 2            # the constant is the measurement, not a loose cover
    assert K.BAR4 == K.FOUR_EMUL + 2e-6 and K.BAR4 < 1e-4


def test_refusals_follow_from_the_launcher():
    for name, kw in K.PRE_REFUSALS:
        assert K.fwd_pre_refuses(**kw), name
    for W in K.PRE_WIDTHS:
        assert not K.fwd_pre_refuses(W)
        assert not K.fwd_pre_refuses(W, pre=False)
    assert not K.fwd_pre_refuses(16, ext=True)
    assert not K.fwd_pre_refuses(8, pre=False) and not K.fwd_pre_refuses(32, pre=False, single=True)
    sb = _src("conv_sb.hip")
    for cond in ("if ((pre_scale || ext_out) && !conv64_fwd_sb_takes_pre(kc, W)) return -3;",
                 "int conv64_fwd_sb_takes_pre(const KernelChoices& kc, int W) { return (W == 16 || W == 4) && !kc.mfma_one; }",
                 "if (kc.mfma_one || !pre_shift || pre_out == x) return -3;", "if (ext_out && !ext_gamma) return -3;",
                 "if (ext_out) return -3;      // window extremes come with the PRE loader only"):
        assert cond in sb, cond
    # the region launchers of W = 4 and W = 8 are handed ext_out, or their refusal could not see it
    assert re.search(r"if \(W == 4\) return launch_sbd<2, 48>\([^;]*pre_out, ext_gamma, ext_out\);", sb)
    assert re.search(r"if \(W == 8\) return launch_sbd<3, 32>\([^;]*ext_gamma, ext_out\);", sb)


def test_activation_is_exact():
    """fma32 against exact rational arithmetic, on draws and on the cases that double rounding would get wrong"""
    rng = np.random.default_rng(7)
    v = K.binade(rng, 4000, -12, 13)
    s = K.binade(rng, 4000, -12, 13)
    t = K.binade(rng, 4000, -12, 13)
    # a product one bit above a float32 tie, the addend far below it: float64 alone rounds p + t to the tie, then to even
    v[:3] = np.float32(1 + 2.0 ** -12)
    s[:3] = np.float32(1 + 2.0 ** -12)
    t[:3] = np.float32([2.0 ** -60, -2.0 ** -60, 0.0])
    got = K.fma32(v, s, t)
    assert got.dtype == np.float32

    def rn32(q):
        """the float32 nearest (ties to even) to the rational q"""
        if q == 0:
            return np.float32(0)
        sign, a = (-1, -q) if q < 0 else (1, q)
        e = math.floor(math.log2(a))
        while Fraction(2) ** e > a:
            e -= 1
        while Fraction(2) ** (e + 1) <= a:
            e += 1
        ulp = Fraction(2) ** (max(e, -126) - 23)
        n = a / ulp
        k = n.numerator // n.denominator
        rem = n - k
        if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and k & 1):
            k += 1
        return np.float32(sign * float(k * ulp))

    for i in range(600):
        want = rn32(Fraction(float(v[i])) * Fraction(float(s[i])) + Fraction(float(t[i])))
        assert got[i] == want, (i, v[i], s[i], t[i], got[i], want)
    a = K.activated(3, 17, 16)
    assert a.dtype == np.float32 and (a >= 0).all() and 0.2 < (a == 0).mean() < 0.8


def test_window_selection_is_exact():
    gamma = K.pre_params()[2]
    z = K.conv32(K.activated(3, 2, 16), K.weights()[0], K.weights()[1])
    e = K.ext_select(z, gamma)
    assert e.shape == (3, 2, 4, 64) and e.dtype == np.float32
    for c in (0, 5, 37, 1):
        for f4 in range(4):
            win = z[1, 1, 4 * f4:4 * f4 + 4, c]
            assert e[1, 1, f4, c] == (win.min() if gamma[c] < 0 else win.max())
    assert (e[..., 37] == z.reshape(3, 2, 4, 4, 64).max(3)[..., 37]).all()      # -0.0 takes the maximum
    # BatchNorm + ReLU are monotone: the pooled tensor is the activation of the selected extreme, bit for bit
    scale2, shift2 = K.pre_params()[3:]
    pooled = K.act32(z, scale2, shift2).reshape(3, 2, 4, 4, 64).max(3)
    assert np.array_equal(K.act32(e, scale2, shift2), pooled)
