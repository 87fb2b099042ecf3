"""The attention operators (seld_attn_*, seld_ln_*: seld_amd/csrc/attention.hip) and the transformer encoder block / stage composed from them
(seld_amd/modules.py; reference modules.py:106-126, 379-407) on the device against the fp64 restatement tests/transformer_oracle.py, at
the project's bar (helpers.check: max|d| / max|ref| <= 1e-4), and models.seldnet with SECOND = transformer_encoder_stage in a test step and
a train step.

One gradient is zero by mathematics: the key bias shifts every logit of a query row by the same amount, which softmax does not see (at
S = 1 the same holds for the query and key inputs).  The rule of tests/test_modules_gpu.py:143-145 applies as written: where the
reference gradient's maximum is below 1e-9 of the largest gradient, |got| <= 1e-3 * the largest gradient is asserted instead."""
import copy
import ctypes as C
import math

import numpy as np
import pytest
import torch

import transformer_oracle as T
from helpers import check, dev, ptr

pytestmark = pytest.mark.gpu


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _check_or_zero(name, got, ref, biggest):
    if np.abs(ref).max() < 1e-9 * biggest:
        assert np.abs(got).max() <= 1e-3 * biggest, name
    else:
        check(name, got, ref)


# ---------------------------------------------------------------- attention
def _attention_run(lib, q, k, v, do, B, S, H, d, scale, fused, save=True):
    """q, k, v, do: numpy [B, S, H, d] -> (o, lse, dq, dk, dv) as numpy; fused: the operands are column slices of one [B*S, 3*H*d + 8] buffer
    (and the gradients of another), else contiguous"""
    HD = H * d
    R = B * S
    if fused:
        ld = 3 * HD + 8
        buf = torch.full((R, ld), float("nan"), device="cuda")
        gbuf = torch.full((R, ld), float("nan"), device="cuda")
        views = [buf[:, i * HD:(i + 1) * HD] for i in range(3)]
        gviews = [gbuf[:, i * HD:(i + 1) * HD] for i in range(3)]
        for t, a in zip(views, (q, k, v)):
            t.copy_(dev(a.reshape(R, HD)))
    else:
        ld = HD
        views = [dev(a.reshape(R, HD)) for a in (q, k, v)]
        gviews = [torch.full((R, HD), float("nan"), device="cuda") for _ in range(3)]
    o = torch.full((R, HD), float("nan"), device="cuda")
    lse = torch.full((B, H, S), float("nan"), device="cuda") if save else None
    rc = lib.seld_attn_fwd(ptr(views[0]), ptr(views[1]), ptr(views[2]), ld, ld, ld, ptr(o), ptr(lse), B, S, H, d, scale, _stream())
    assert rc == 0
    if not save:
        torch.cuda.synchronize()
        return o.cpu().numpy()
    n = lib.seld_attn_bwd_scratch(B, S, H, d)
    scratch = torch.full((n,), float("nan"), device="cuda")
    god = dev(do.reshape(R, HD))
    rc = lib.seld_attn_bwd(ptr(views[0]), ptr(views[1]), ptr(views[2]), ld, ld, ld, ptr(o), ptr(god), ptr(lse), ptr(gviews[0]), ptr(gviews[1]),
                           ptr(gviews[2]), ld, ld, ld, ptr(scratch), B, S, H, d, scale, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    if fused:      # the columns between and behind the slices were not touched
        assert bool(torch.isnan(gbuf[:, 3 * HD:]).all()) and bool(torch.isnan(buf[:, 3 * HD:]).all())
    return [o.cpu().numpy(), lse.cpu().numpy()] + [g.contiguous().cpu().numpy() for g in gviews]


@pytest.mark.parametrize("B,S,H,d", [(2, 600, 4, 32), (3, 61, 4, 24), (2, 130, 4, 48), (1, 1, 2, 8)])
def test_attention_forward_and_backward(seld_lib, B, S, H, d):
    rng = np.random.default_rng(S)
    q, k, v, do = (rng.standard_normal((B, S, H, d)) for _ in range(4))
    scale = 1.0 / math.sqrt(d)
    tq, tk, tv = (torch.tensor(a, requires_grad=True) for a in (q, k, v))
    o_ref, lse_ref = T.attention(tq, tk, tv, scale)
    gq, gk, gv = torch.autograd.grad((o_ref * torch.tensor(do)).sum(), (tq, tk, tv))
    R, HD = B * S, H * d
    biggest = max(float(g.abs().max()) for g in (gq, gk, gv))
    runs = {}
    for fused in (False, True):
        got = runs[fused] = _attention_run(seld_lib, q, k, v, do, B, S, H, d, scale, fused)
        tag = f"attention {'fused' if fused else 'contiguous'} "
        check(tag + "O", got[0], o_ref.detach().numpy().reshape(R, HD))
        check(tag + "lse", got[1], lse_ref.detach().numpy())
        for name, g, r in zip(("dQ", "dK", "dV"), got[2:], (gq, gk, gv)):
            _check_or_zero(tag + name, g, r.numpy().reshape(R, HD), biggest)      # S = 1: dQ = dK = 0 exactly
    # the strides change addresses only; a second run gives the same bits; so does the forward without the log-sum-exp
    for a, b in zip(runs[False], runs[True]):
        assert np.array_equal(a, b)
    again = _attention_run(seld_lib, q, k, v, do, B, S, H, d, scale, False)
    for a, b in zip(runs[False], again):
        assert np.array_equal(a, b)
    assert np.array_equal(_attention_run(seld_lib, q, k, v, do, B, S, H, d, scale, False, save=False), runs[False][0])


# ---------------------------------------------------------------- attention: every head width, tile edge, stride and softmax regime
NAN_BITS = 0x7FC00000      # torch.full(..., nan): every sentinel float holds these bits until a kernel writes it


def _bits(t):
    return t.view(torch.int32)


class _Window:
    """[rows, cols] floats at row stride ld, `front` floats into a NaN-filled allocation of front + rows * span + back floats (span >= ld: the
    widest stride of the call, so that a kernel that took another operand's stride stays inside the allocation and reads or writes sentinels)"""

    def __init__(self, rows, cols, ld=None, span=None, front=0, back=0, data=None):
        ld = cols if ld is None else ld
        span = ld if span is None else span
        assert span >= ld >= cols
        self.buf = torch.full((front + rows * span + back,), float("nan"), device="cuda")
        self.view = torch.as_strided(self.buf, (rows, cols), (ld, 1), front)
        self.ld = ld
        self.outside = torch.ones(self.buf.numel(), dtype=torch.bool, device="cuda")
        torch.as_strided(self.outside, (rows, cols), (ld, 1), front).fill_(False)
        if data is not None:
            self.view.copy_(dev(np.asarray(data).reshape(rows, cols)))
        assert self.view.data_ptr() == self.buf.data_ptr() + 4 * front

    def ptr(self):
        return C.c_void_p(self.view.data_ptr())

    def snapshot(self):
        self.saved = _bits(self.buf).clone()

    def assert_unchanged(self, name):
        assert torch.equal(_bits(self.buf), self.saved), f"{name}: an input, or the band around it, was written"

    def assert_band(self, name):
        assert bool((_bits(self.buf)[self.outside] == NAN_BITS).all()), f"{name}: a float outside the [rows, cols] window was written"

    def numpy(self):
        return self.view.contiguous().cpu().numpy()


def _attention_padded(lib, q, k, v, do, B, S, H, d, scale, lds=None, fronts=None, save=True):
    """as _attention_run, with every operand inside a larger NaN-filled allocation.  lds: the row strides of Q, K, V, dQ, dK, dV (None: H * d,
    contiguous); fronts: the floats in front of each of those six views (None: the band).  O, lse, dO and the delta scratch have a band of
    64 * H * d + 1 floats (odd: no base pointer is aligned beyond 4 bytes) in front and behind; so have the six strided operands.  After the calls
    every float outside the windows still holds the sentinel's bits, and Q, K, V, dO, O and lse hold the bits they had in front of the backward."""
    HD, R = H * d, B * S
    band = 64 * HD + 1
    lds = [HD] * 6 if lds is None else list(lds)
    fronts = [band] * 6 if fronts is None else list(fronts)
    span = max(lds)
    wq, wk, wv = (_Window(R, HD, ld, span, f, band, a) for ld, f, a in zip(lds[:3], fronts[:3], (q, k, v)))
    gq, gk, gv = (_Window(R, HD, ld, span, f, band) for ld, f in zip(lds[3:], fronts[3:]))
    wo = _Window(R, HD, front=band, back=band)
    wl = _Window(B * H, S, front=band, back=band)
    rc = lib.seld_attn_fwd(wq.ptr(), wk.ptr(), wv.ptr(), lds[0], lds[1], lds[2], wo.ptr(), wl.ptr() if save else None, B, S, H, d, scale, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    wo.assert_band("O")
    if not save:
        assert bool((_bits(wl.buf) == NAN_BITS).all())
        return wo.numpy()
    wl.assert_band("lse")
    n = lib.seld_attn_bwd_scratch(B, S, H, d)
    assert n == B * H * S
    wd = _Window(1, n, front=band, back=band)
    wg = _Window(R, HD, front=band, back=band, data=do)
    inputs = {"Q": wq, "K": wk, "V": wv, "dO": wg, "O": wo, "lse": wl}
    for w in inputs.values():
        w.snapshot()
    rc = lib.seld_attn_bwd(wq.ptr(), wk.ptr(), wv.ptr(), lds[0], lds[1], lds[2], wo.ptr(), wg.ptr(), wl.ptr(), gq.ptr(), gk.ptr(), gv.ptr(), lds[3],
                           lds[4], lds[5], wd.ptr(), B, S, H, d, scale, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    for name, w in inputs.items():
        w.assert_unchanged(name)
    for name, w in (("dQ", gq), ("dK", gk), ("dV", gv), ("delta scratch", wd)):
        w.assert_band(name)
    assert bool(torch.isfinite(wd.view).all())      # delta is written for every (batch, head, query)
    return [wo.numpy(), wl.numpy().reshape(B, H, S), gq.numpy(), gk.numpy(), gv.numpy()]


def _odd_strides(HD):
    """six different row strides, none a multiple of 4 floats, and six different odd offsets of the views into their allocations"""
    lds = [HD + e for e in (1, 3, 5, 7, 9, 11)]
    lds = [ld + 1 if ld % 4 == 0 else ld for ld in lds]      # H * d is a multiple of 8 here, so this never fires; kept as the rule
    assert len(set(lds)) == 6 and all(ld % 4 for ld in lds)
    return lds, [64 * HD + o for o in (1, 3, 5, 7, 9, 11)]


def _attention_reference(q, k, v, do, scale):
    """the fp64 oracle on the fp32-rounded inputs, batch by batch (attention is independent per batch; the [H, S, S] logits of one batch are
    all that is alive) -> (o [R, HD], lse [B, H, S], dq, dk, dv [R, HD])"""
    B, S, H, d = q.shape
    outs = [[] for _ in range(5)]
    for b in range(B):
        tq, tk, tv = (torch.tensor(T.f32(a[b:b + 1]), requires_grad=True) for a in (q, k, v))
        o, lse = T.attention(tq, tk, tv, scale)
        g = torch.autograd.grad((o * torch.tensor(T.f32(do[b:b + 1]))).sum(), (tq, tk, tv))
        for lst, t in zip(outs, (o.detach(), lse.detach()) + g):
            lst.append(t.numpy())
    o, lse, gq, gk, gv = (np.concatenate(x, 0) for x in outs)
    return [o.reshape(B * S, H * d), lse] + [g.reshape(B * S, H * d) for g in (gq, gk, gv)]


NAMES = ("O", "lse", "dQ", "dK", "dV")


def _compare(tag, got, ref, B, S, H, d, last_tile=False, per_head=False):
    """helpers.check on each whole tensor (the zero-gradient rule where the mathematics gives 0: S = 1); last_tile: also the rows of the last
    64-row tile alone; per_head: also every (batch, head) slice alone, so that a small head is not measured against a large one"""
    biggest = max(np.abs(r).max() for r in ref[2:])
    worst = 0.0
    for name, g, r in zip(NAMES, got, ref):
        if name in ("dQ", "dK") and np.abs(r).max() < 1e-9 * biggest:
            _check_or_zero(f"{tag} {name}", g, r, biggest)
            continue
        worst = max(worst, check(f"{tag} {name}", g, r))
        if name == "lse":
            g4, r4 = g[:, :, :, None], r[:, :, :, None]                              # [B, H, S, 1]
        else:
            g4, r4 = (a.reshape(B, S, H, d).transpose(0, 2, 1, 3) for a in (g, r))     # [B, H, S, d]
        if last_tile:
            s0 = 64 * ((S - 1) // 64)
            worst = max(worst, check(f"{tag} {name} rows >= {s0}", g4[:, :, s0:], r4[:, :, s0:]))
        if per_head:
            for b in range(B):
                for h in range(H):
                    worst = max(worst, check(f"{tag} {name} b{b} h{h}", g4[b, h], r4[b, h]))
    print(f"[worst] {tag}: {worst:.3e}")
    return worst


def _unit_normal(B, S, H, d, seed):
    rng = np.random.default_rng(seed)
    return [T.f32(rng.standard_normal((B, S, H, d))) for _ in range(4)]


@pytest.mark.parametrize("d", [8, 16, 24, 32, 40, 48, 56, 64])
def test_attention_every_head_width_contiguous_and_odd_strides(seld_lib, d):
    """all eight template instantiations at a multi-tile ragged S and an odd H; the strided run has six different row strides, none a
    multiple of 4 floats, on views that start an odd number of floats into their allocations, and gives the contiguous run's bits"""
    B, S, H = 2, 150, 3
    q, k, v, do = _unit_normal(B, S, H, d, 1000 + d)
    scale = 1.0 / math.sqrt(d)
    ref = _attention_reference(q, k, v, do, scale)
    plain = _attention_padded(seld_lib, q, k, v, do, B, S, H, d, scale)
    _compare(f"d sweep d={d} contiguous", plain, ref, B, S, H, d, last_tile=True)
    lds, fronts = _odd_strides(H * d)
    strided = _attention_padded(seld_lib, q, k, v, do, B, S, H, d, scale, lds, fronts)
    _compare(f"d sweep d={d} strided", strided, ref, B, S, H, d)
    for name, a, b in zip(NAMES, plain, strided):
        assert np.array_equal(a, b), name
    assert np.array_equal(_attention_padded(seld_lib, q, k, v, do, B, S, H, d, scale, save=False), plain[0])
    assert np.array_equal(_attention_padded(seld_lib, q, k, v, do, B, S, H, d, scale, lds, fronts, save=False), plain[0])


@pytest.mark.parametrize("d", [16, 40])
@pytest.mark.parametrize("S", [2, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 192])
def test_attention_tile_edges(seld_lib, S, d):
    """S around the 32-key half tile and the 64-row tile, at a head width with one 32-column block and one with a partly dead second block;
    the rows of the last tile are also checked alone"""
    B, H = 2, 2
    q, k, v, do = _unit_normal(B, S, H, d, 2000 + 100 * S + d)
    scale = 1.0 / math.sqrt(d)
    ref = _attention_reference(q, k, v, do, scale)
    got = _attention_padded(seld_lib, q, k, v, do, B, S, H, d, scale)
    _compare(f"edge S={S} d={d}", got, ref, B, S, H, d, last_tile=True)
    lds, fronts = _odd_strides(H * d)
    for name, a, b in zip(NAMES, got, _attention_padded(seld_lib, q, k, v, do, B, S, H, d, scale, lds, fronts)):
        assert np.array_equal(a, b), name


@pytest.mark.parametrize("B,S,H,d", [(3, 70, 2, 24), (1, 1, 1, 8), (2, 64, 1, 64), (1, 65, 5, 8)])
def test_attention_guard_bands_and_distinct_strides(seld_lib, B, S, H, d):
    """the bands of _attention_padded at small shapes (one row; one full tile of the widest head; one row into a second tile), with the strides
    in the reverse order of the d sweep: swapping any two of them moves an operand"""
    q, k, v, do = _unit_normal(B, S, H, d, 3000 + S)
    scale = 1.0 / math.sqrt(d)
    ref = _attention_reference(q, k, v, do, scale)
    plain = _attention_padded(seld_lib, q, k, v, do, B, S, H, d, scale)
    _compare(f"bands {B},{S},{H},{d} contiguous", plain, ref, B, S, H, d)
    lds, fronts = _odd_strides(H * d)
    strided = _attention_padded(seld_lib, q, k, v, do, B, S, H, d, scale, lds[::-1], fronts[::-1])
    for name, a, b in zip(NAMES, plain, strided):
        assert np.array_equal(a, b), name


@pytest.mark.parametrize("scale", [0.37, 1.0])
def test_attention_scale_is_the_argument(seld_lib, scale):
    """d = 24: 1 / sqrt(d) = 0.204 is neither"""
    B, S, H, d = 2, 100, 2, 24
    q, k, v, do = _unit_normal(B, S, H, d, 4000)
    ref = _attention_reference(q, k, v, do, scale)
    _compare(f"scale {scale}", _attention_padded(seld_lib, q, k, v, do, B, S, H, d, scale), ref, B, S, H, d)


@pytest.mark.parametrize("kind,span,B,S,H,d", T.STRESS_CASES, ids=lambda v: str(v))
def test_attention_peaked_and_extreme_softmax(seld_lib, kind, span, B, S, H, d):
    """the deterministic stress inputs of transformer_oracle.stress_qkv (tests/test_attention_cpu.py: a plain fp32 evaluation is within 5e-5
    of the oracle on each of them, so a miss of 1e-4 here is the kernel's).  Whole tensors under the project's metric, as everywhere.  Not
    asserted per slice: under ramp_down the last tile's keys have gradients of 1e-40 (nothing to measure), and at span 100 the dQ of one (batch,
    head) slice whose maximum is 0.62 of the tensor's measured 1.3e-4 of its own maximum on an MI355X (8.1e-5 of the tensor's; a plain fp32
    evaluation on the CPU: 1.8e-5): component 0 of dQ is a sum over keys of dS * 200 that cancels to a few units, and each logit of about
    100 carries the roundings of its d / 2 accumulation steps at ulp(100) = 7.6e-6.  Device figures: DESIGN.md section 3e."""
    q, k, v, do, scale = T.stress_qkv(kind, span, B, S, H, d)
    ref = _attention_reference(q, k, v, do, scale)
    assert min(np.abs(r).max() for r in ref[2:]) > 1e-2      # no gradient vanishes: there is something to check
    got = _attention_padded(seld_lib, q, k, v, do, B, S, H, d, scale)
    _compare(f"stress {kind} span={span} d={d}", got, ref, B, S, H, d)


@pytest.mark.parametrize("H", [1, 5])
def test_attention_unequal_heads(seld_lib, H):
    """V and dO of head h are 10^h times unit-normal: every (batch, head) slice is checked against its own maximum"""
    B, S, d = 2, 100, 16
    q, k, v, do = _unit_normal(B, S, H, d, 5000 + H)
    gain = (10.0 ** np.arange(H))[None, None, :, None]
    v, do = T.f32(v * gain), T.f32(do * gain)
    scale = 1.0 / math.sqrt(d)
    ref = _attention_reference(q, k, v, do, scale)
    _compare(f"heads H={H}", _attention_padded(seld_lib, q, k, v, do, B, S, H, d, scale), ref, B, S, H, d, per_head=True)


@pytest.mark.parametrize("d", [24, 48])
def test_attention_bench_shape(seld_lib, d):
    """the measured shapes (32, 600, 4, 24 | 48): a large B in the grid's (tile, head, batch) decomposition"""
    B, S, H = 32, 600, 4
    q, k, v, do = _unit_normal(B, S, H, d, 6000 + d)
    scale = 1.0 / math.sqrt(d)
    ref = _attention_reference(q, k, v, do, scale)
    _compare(f"bench shape d={d}", _attention_padded(seld_lib, q, k, v, do, B, S, H, d, scale), ref, B, S, H, d, last_tile=True, per_head=(d == 24))


# ---------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("rows,Cc", [(7, 8), (1200, 128), (60, 4378), (3, 1)])
def test_layer_norm_forward_and_backward(seld_lib, rows, Cc, residual):
    lib = seld_lib
    rng = np.random.default_rng(rows + Cc)
    x, r, dy = rng.standard_normal((rows, Cc)) * 2 + 0.5, rng.standard_normal((rows, Cc)), rng.standard_normal((rows, Cc))
    gamma, beta = 1 + 0.3 * rng.standard_normal(Cc), 0.2 * rng.standard_normal(Cc)
    tx, tr_, tg, tb = (torch.tensor(a, requires_grad=True) for a in (x, r, gamma, beta))
    y_ref = T.layer_norm(tx + tr_ if residual else tx, tg, tb)
    gx, gg, gb = torch.autograd.grad((y_ref * torch.tensor(dy)).sum(), (tx, tg, tb))
    dx_, dr_, dg_, db_, ddy = dev(x), dev(r) if residual else None, dev(gamma), dev(beta), dev(dy)
    y, xhat, rstd, dz = (torch.full(s, float("nan"), device="cuda") for s in ((rows, Cc), (rows, Cc), (rows,), (rows, Cc)))
    dgamma, dbeta = torch.full((Cc,), float("nan"), device="cuda"), torch.full((Cc,), float("nan"), device="cuda")
    scratch = torch.full((lib.seld_ln_scratch(rows, Cc),), float("nan"), device="cuda")
    assert lib.seld_ln_fwd(ptr(dx_), ptr(dr_), ptr(dg_), ptr(db_), T.LN_EPS, ptr(y), ptr(xhat), ptr(rstd), rows, Cc, _stream()) == 0
    assert lib.seld_ln_bwd(ptr(ddy), ptr(xhat), ptr(rstd), ptr(dg_), ptr(dz), ptr(dgamma), ptr(dbeta), ptr(scratch), rows, Cc, _stream()) == 0
    y2 = torch.full((rows, Cc), float("nan"), device="cuda")
    assert lib.seld_ln_fwd(ptr(dx_), ptr(dr_), ptr(dg_), ptr(db_), T.LN_EPS, ptr(y2), None, None, rows, Cc, _stream()) == 0
    torch.cuda.synchronize()
    check("LayerNorm y", y.cpu().numpy(), y_ref.detach().numpy())
    assert torch.equal(y, y2)      # the inference form (nothing saved) gives the same bits
    if Cc == 1:
        # one feature: xhat = 0, y = beta, and the input's gradient is 0 exactly
        assert float(dz.abs().max()) <= 1e-3 * float(np.abs(dy).max()) and float(gx.abs().max()) < 1e-12
        assert float(dgamma.abs().max()) <= 1e-3 * float(gb.abs().max())
    else:
        check("LayerNorm dz", dz.cpu().numpy(), gx.numpy())
        check("LayerNorm dgamma", dgamma.cpu().numpy(), gg.numpy())
    check("LayerNorm dbeta", dbeta.cpu().numpy(), gb.numpy())


def _layer_norm_padded(lib, x, r, gamma, beta, dy):
    """seld_ln_fwd (saving and not saving) and seld_ln_bwd twice on numpy inputs (r None: no residual), every output and the scratch inside
    NaN-filled allocations with a band in front and behind -> (y, xhat, rstd, dz, dgamma, dbeta) as numpy.  Asserted here: the bands and the
    floats behind seld_ln_scratch(rows, C) keep the sentinel's bits, the inputs keep theirs, the inference form gives the same y, and the two
    backward runs (each on a freshly NaN-filled scratch) give the same bits."""
    rows, Cc = x.shape
    band = 64 * Cc + 1
    mk = lambda n, m, data=None: _Window(n, m, front=band, back=band, data=data)
    ins = {"x": mk(rows, Cc, x), "gamma": mk(1, Cc, gamma), "beta": mk(1, Cc, beta), "dy": mk(rows, Cc, dy)}
    if r is not None:
        ins["r"] = mk(rows, Cc, r)
    y, y2, xhat, rstd = mk(rows, Cc), mk(rows, Cc), mk(rows, Cc), mk(1, rows)
    n = lib.seld_ln_scratch(rows, Cc)
    assert 2 * Cc <= n <= 256 * 2 * Cc
    for w in ins.values():
        w.snapshot()
    rp = ins["r"].ptr() if r is not None else None
    assert lib.seld_ln_fwd(ins["x"].ptr(), rp, ins["gamma"].ptr(), ins["beta"].ptr(), T.LN_EPS, y.ptr(), xhat.ptr(), rstd.ptr(), rows, Cc, _stream()) == 0
    assert lib.seld_ln_fwd(ins["x"].ptr(), rp, ins["gamma"].ptr(), ins["beta"].ptr(), T.LN_EPS, y2.ptr(), None, None, rows, Cc, _stream()) == 0
    torch.cuda.synchronize()
    ins["xhat"], ins["rstd"] = xhat, rstd
    for name, w in (("y", y), ("y, nothing saved", y2), ("xhat", xhat), ("rstd", rstd)):
        w.assert_band(name)
    xhat.snapshot()
    rstd.snapshot()
    assert torch.equal(_bits(y.view), _bits(y2.view))      # the inference form (nothing saved) gives the same bits
    runs = []
    for _ in range(2):
        dz, dgamma, dbeta, scratch = mk(rows, Cc), mk(1, Cc), mk(1, Cc), mk(1, n)
        assert lib.seld_ln_bwd(ins["dy"].ptr(), xhat.ptr(), rstd.ptr(), ins["gamma"].ptr(), dz.ptr(), dgamma.ptr(), dbeta.ptr(), scratch.ptr(), rows,
                               Cc, _stream()) == 0
        torch.cuda.synchronize()
        for name, w in (("dz", dz), ("dgamma", dgamma), ("dbeta", dbeta), ("scratch", scratch)):
            w.assert_band(name)
        runs.append([dz.numpy(), dgamma.numpy()[0], dbeta.numpy()[0]])
    for name, w in ins.items():
        w.assert_unchanged(name)
    for a, b in zip(*runs):
        assert np.array_equal(a, b)      # a fixed summation order
    return [y.numpy(), xhat.numpy(), rstd.numpy()[0]] + runs[0]


def _layer_norm_reference(x, r, gamma, beta, dy):
    """the fp64 oracle on the fp32-rounded inputs -> (y, xhat, rstd, dz, dgamma, dbeta)"""
    tx, tg, tb = (torch.tensor(T.f32(a), requires_grad=True) for a in (x, gamma, beta))
    z = tx + torch.tensor(T.f32(r)) if r is not None else tx
    y = T.layer_norm(z, tg, tb)
    gx, gg, gb = torch.autograd.grad((y * torch.tensor(T.f32(dy))).sum(), (tx, tg, tb))
    zd = z.detach()
    rstd = 1.0 / torch.sqrt(zd.var(dim=-1, unbiased=False) + T.LN_EPS)
    xhat = (zd - zd.mean(dim=-1, keepdim=True)) * rstd[:, None]
    return [t.numpy() for t in (y.detach(), xhat, rstd, gx, gg, gb)]


def _layer_norm_case(lib, tag, x, r, gamma, beta, dy):
    ref = _layer_norm_reference(x, r, gamma, beta, dy)
    got = _layer_norm_padded(lib, x, r, gamma, beta, dy)
    worst = max(check(f"{tag} {name}", g, f) for name, g, f in zip(("y", "xhat", "rstd", "dz", "dgamma", "dbeta"), got, ref))
    print(f"[worst] {tag}: {worst:.3e}")
    return got, ref


def _plain_rows(rows, Cc, seed):
    rng = np.random.default_rng(seed)
    x, r, dy = rng.standard_normal((rows, Cc)) * 2 + 0.5, rng.standard_normal((rows, Cc)), rng.standard_normal((rows, Cc))
    return x, r, 1 + 0.3 * rng.standard_normal(Cc), 0.2 * rng.standard_normal(Cc), dy


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("rows,Cc", [(16, 8), (17, 8), (4096, 8), (4097, 8), (4100, 8), (19200, 8), (19200, 128), (19200, 192)])
def test_layer_norm_row_counts_around_the_capped_reduction(seld_lib, rows, Cc, residual):
    """the dgamma / dbeta first stage has ceil(rows / 16) workgroups up to 4096 rows and 256 beyond: 4100 rows leave workgroups 242 .. 255
    without a row (they still write zeros over the NaN scratch), 19 200 is the bench shape's row count"""
    x, r, gamma, beta, dy = _plain_rows(rows, Cc, 7000 + rows + Cc)
    _layer_norm_case(seld_lib, f"LayerNorm rows={rows} C={Cc}", x, r if residual else None, gamma, beta, dy)


@pytest.mark.parametrize("Cc", [2, 63, 64, 65, 255, 256, 257])
def test_layer_norm_columns_around_the_wave_and_the_workgroup(seld_lib, Cc):
    x, r, gamma, beta, dy = _plain_rows(50, Cc, 8000 + Cc)
    _layer_norm_case(seld_lib, f"LayerNorm C={Cc}", x, r, gamma, beta, dy)


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("mean,std,rows,Cc", T.LN_OFFSET_CASES)
def test_layer_norm_offset_rows(seld_lib, mean, std, rows, Cc, residual):
    """transformer_oracle.offset_rows: rows far from 0 (a one-pass fp32 variance misses the bar on them: tests/test_attention_cpu.py), one row
    that the residual makes exactly constant and one constant on its own (y = beta there, rstd = 1 / sqrt(eps)), gamma over three decades,
    beta at 50.  Without the residual the input is the fp32 sum x + r."""
    x, r, dy, gamma, beta = T.offset_rows(mean, std, rows, Cc)
    if not residual:
        x, r = T.f32(x + r), None
    got, ref = _layer_norm_case(seld_lib, f"LayerNorm offset mean={mean} C={Cc}", x, r, gamma, beta, dy)
    # the constant rows have the largest rstd (and with it the largest dz): the other rows against their own maximum as well
    check("LayerNorm offset rstd of the other rows", got[2][3:], ref[2][3:])
    check("LayerNorm offset dz of the other rows", got[3][3:], ref[3][3:])
    for row in (1, 2):
        assert np.abs(ref[0][row] - beta).max() == 0.0 and abs(ref[2][row] - 1.0 / math.sqrt(T.LN_EPS)) < 1e-9
        check(f"LayerNorm constant row {row} y", got[0][row], beta)
        check(f"LayerNorm constant row {row} rstd", got[2][row:row + 1], ref[2][row:row + 1])
        check(f"LayerNorm constant row {row} dz", got[3][row], ref[3][row])


# ---------------------------------------------------------------- the block and the stage
def _stage_case(B, S, D, H, dk, ffm, k, depth, seed, activation="relu"):
    from oracle import seldnet_oracle as O
    from seld_amd import modules
    cfg = {"depth": depth, "n_head": H, "key_dim": dk, "ff_multiplier": ffm, "kernel_size": k, "dropout_rate": 0, "activation": activation}
    stage = (modules.transformer_encoder_stage if depth > 1 else modules.transformer_encoder_block)(cfg)((B, S, D))
    rt = stage.blocks[0].rt
    rt.finalize()
    specs = T.stage_specs(D, cfg, depth)
    assert [(n, s) for n, _, s in rt.variables] == specs and rt.n_state == 0
    w = T.random_block_weights(specs, seed)
    rng = np.random.default_rng(seed)
    x, dy = rng.standard_normal((B, S, D)), rng.standard_normal((B, S, D))
    rt.params[:rt.n_params].copy_(torch.as_tensor(w))
    xd = dev(x.reshape(B * S, D))
    out = stage.forward(xd, B, True).cpu().numpy().copy()
    out_eval = stage.forward(xd, B, False).cpu().numpy().copy()
    stage.forward(xd, B, True)
    dx = stage.backward(dev(dy.reshape(B * S, D)), B).cpu().numpy().copy()
    grads = rt.grads[:rt.n_params].cpu().numpy().copy()
    fw = torch.tensor(w, dtype=torch.float64, requires_grad=True)
    xt = torch.tensor(x, requires_grad=True)
    yt = T.stage_forward(xt, O.unflatten(fw, specs), cfg, depth)
    gw, gx = torch.autograd.grad((yt * torch.tensor(dy)).sum(), (fw, xt))
    check("transformer forward", out, yt.detach().numpy().reshape(B * S, D))
    assert np.array_equal(out, out_eval)      # no dropout, no batch statistics: training and inference agree bit for bit
    check("transformer input gradient", dx, gx.numpy().reshape(B * S, D))
    off, biggest = 0, float(gw.abs().max())
    for n, s in specs:
        kk = int(np.prod(s))
        _check_or_zero(f"transformer grad {n}", grads[off:off + kk], gw.numpy()[off:off + kk], biggest)
        off += kk


@pytest.mark.parametrize("B,S,D,H,dk,ffm,k", [(2, 600, 128, 4, 32, 2, 1), (3, 61, 96, 4, 24, 4, 3)])
def test_transformer_encoder_block(B, S, D, H, dk, ffm, k):
    _stage_case(B, S, D, H, dk, ffm, k, depth=1, seed=S)


@pytest.mark.parametrize("B,S,D,H,dk,ffm,k", [(2, 70, 50, 3, 8, 1.5, 2), (2, 33, 40, 2, 64, 2, 4), (3, 1, 48, 3, 16, 2, 3)])
def test_transformer_encoder_block_odd_configurations(B, S, D, H, dk, ffm, k):
    """what the reference allows and the rows above do not have: n_head * key_dim below and above d_model, a d_model that is no multiple of
    8, a fractional ff_multiplier * d_model (int() of it), an even kernel_size (TensorFlow's 'same' then pads one frame more behind than in
    front), the widest head, and a single frame (S = 1: the query and key projections have no gradient)"""
    _stage_case(B, S, D, H, dk, ffm, k, depth=1, seed=100 + S)


def test_transformer_encoder_stage_of_two_blocks():
    _stage_case(3, 61, 96, 4, 24, 4, 3, depth=2, seed=4, activation="swish")


# ---------------------------------------------------------------- the model
@pytest.mark.parametrize("doa_loss", ["MSE", "MMSE"])
def test_train_step_with_a_transformer_encoder_stage(seldnet_config, doa_loss):
    """models.seldnet with FIRST = mother_stage (the arguments of test_train_step_with_a_mother_stage_first_block) and SECOND =
    transformer_encoder_stage: one test step and one train step against the fp64 oracle — variable list, outputs, both losses, every
    gradient, BatchNorm state, post-Adam weights — then a batch of 2 on the model built for 3"""
    from oracle import seldnet_oracle as O
    from seld_amd import losses, models, train
    from test_modules_gpu import STAGE_FIRST
    cfg = copy.deepcopy(seldnet_config)
    cfg["FIRST"], cfg["FIRST_ARGS"] = "mother_stage", copy.deepcopy(STAGE_FIRST)
    cfg["SECOND"] = "transformer_encoder_stage"
    cfg["SECOND_ARGS"] = {"depth": 2, "n_head": 4, "key_dim": 24, "ff_multiplier": 2, "kernel_size": 1, "dropout_rate": 0}
    B, T_ = 3, 100
    in_shape = (B, T_, 64, 7)
    tr, nt = T.variable_specs(cfg, in_shape)
    w, st = T.random_weights(cfg, in_shape, seed=11)
    x, ys, yd = O.synthetic_batch(B, T_, seed=23)
    model = models.seldnet(in_shape, cfg)
    assert type(model).__name__ == "ComposedSeldNet"
    assert [(n, s) for n, _, s in model.variables] == tr and [(n, s) for n, _, s in model.state_variables] == nt
    assert sum(n.startswith("tf") for n, _ in tr) == 32 and not any(n.startswith("gru") for n, _ in tr)
    model.set_weights(w, st)
    fw = torch.tensor(w, dtype=torch.float64)
    sed_t, doa_t, _ = T.forward(cfg, O.unflatten(fw, tr), O.unflatten(torch.tensor(st, dtype=torch.float64), nt), torch.tensor(x, dtype=torch.float64), False)
    y_t, sl_t, dl_t = train.teststep(model, x, (ys, yd), losses.BinaryCrossentropy(), losses.get_doa_loss(doa_loss))
    check("transformer model teststep sed", y_t[0].cpu().numpy(), sed_t.numpy())
    check("transformer model teststep doa", y_t[1].cpu().numpy(), doa_t.numpy())
    ref = T.train_step(cfg, in_shape, w, st, x, ys, yd, doa_loss=doa_loss, loss_weight=(1.0, 1000.0), lr=1e-3, step=1)
    y_p, sl, dl = train.trainstep(model, x, (ys, yd), losses.BinaryCrossentropy(), losses.get_doa_loss(doa_loss), (1.0, 1000.0), train.Adam(1e-3))
    check("transformer model trainstep sed", y_p[0].cpu().numpy(), ref["sed"])
    check("transformer model trainstep doa", y_p[1].cpu().numpy(), ref["doa"])
    check("transformer model sloss", sl.cpu().numpy(), ref["sloss"])
    check("transformer model dloss", dl.cpu().numpy(), ref["dloss"])
    g = model.get_grads()
    for n, off, sh in model.variables:
        k = int(np.prod(sh))
        r = ref["grad"][off:off + k]
        if np.abs(r).max() < 1e-9 * np.abs(ref["grad"]).max():      # conv biases in front of training-mode BatchNormalization; the key biases
            assert np.abs(g[off:off + k]).max() <= 1e-3 * np.abs(ref["grad"]).max(), n
            continue
        check(f"transformer model grad {n}", g[off:off + k], r)
    w1, st1 = model.get_weights()
    check("transformer model BN state", st1, ref["new_state"])
    big = np.abs(ref["grad"]) > 1e-3 * np.abs(ref["grad"]).max()
    assert np.abs(w1 - ref["new_w"])[big].max() <= 2e-3 * 1e-3 + 1e-7       # Adam's first step moves a weight by lr g / (|g| + eps)
    # a batch of 2 on the model built for 3
    y2 = model(x[:2], training=False)
    sed2, doa2, _ = T.forward(cfg, O.unflatten(torch.tensor(w1, dtype=torch.float64), tr), O.unflatten(torch.tensor(st1, dtype=torch.float64), nt),
                              torch.tensor(x[:2], dtype=torch.float64), False)
    assert tuple(y2[0].shape) == (2, T_ // 5, 12)
    check("transformer model batch of 2 sed", y2[0].cpu().numpy(), sed2.numpy())
    check("transformer model batch of 2 doa", y2[1].cpu().numpy(), doa2.numpy())
    y3, _, _ = train.trainstep(model, x[:2], (ys[:2], yd[:2]), losses.BinaryCrossentropy(), losses.get_doa_loss(doa_loss), (1.0, 1000.0), train.Adam(1e-3))
    assert tuple(y3[1].shape) == (2, T_ // 5, 36) and bool(torch.isfinite(y3[0]).all()) and np.isfinite(model.get_grads()).all()
