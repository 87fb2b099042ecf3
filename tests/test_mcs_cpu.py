"""transforms.mcs_aug without a device: the literal oracle (tests/mcs_oracle.py) on the cases the GPU test runs, the four facts that let one
kernel restate it, and the argument checks of the entry points, which return before anything is enqueued."""
import ctypes as C
import math
import os
import re

import pytest
import torch

import mcs_oracle as O
from conftest import ROOT

INVALID, UNSUPPORTED = -1, -2
_results = {}


def oracle(name):
    """one oracle run per case and session, shared and left unchanged"""
    if name not in _results:
        x, iteration = O.case_input(name)
        trace = []
        _results[name] = (x, iteration, O.mcs(x, iteration, trace=trace), trace)
    return _results[name]


@pytest.mark.parametrize("name", list(O.CASES))
def test_oracle_is_nan_free_and_decisions_have_a_margin(name):
    """no finite cond within a factor 1.25 of 1e6: every is_invertible decision is then the same for any cond computed to better than 25 %.
    The margin is fixed; a case that violates it gets another seed."""
    x, iteration, r, _ = oracle(name)
    assert r["out"].shape == x.shape and r["lam"].shape == x.shape[:3]
    assert r["stab_adds"].shape == (x.shape[0], x.shape[2], 2, iteration + 1)
    assert not torch.isnan(r["out"]).any() and not torch.isnan(r["lam"]).any() and not torch.isnan(r["conds"]).any()
    fin = r["conds"][torch.isfinite(r["conds"])]
    margin = float(torch.maximum(fin / O.EPS_INV, O.EPS_INV / fin).min())
    print(f"{name}: closest finite cond is a factor {margin:.3g} from 1e6; additions seen {sorted(set(r['stab_adds'].flatten().tolist()))}")
    assert margin >= O.MARGIN


def test_cases_reach_what_they_are_named_for():
    assert set(oracle("single_frame")[2]["stab_adds"][:, :, 0].flatten().tolist()) == {2}                # rank 1: class y adds in every call
    assert (oracle("rank_deficient")[2]["stab_adds"][:, :, 0] == 2).all()                              # T < C: two additions each
    masked = oracle("masked")[2]["stab_adds"][0]
    assert (masked[1] >= 1).any() and (masked[2, 0] >= 2).all()                                         # the zero and the constant column
    lam = oracle("one_channel")[2]["lam"]
    assert float((lam - 0.5).abs().max()) <= 4 * 2.0 ** -53


@pytest.mark.parametrize("name", list(O.CASES))
def test_order_of_the_time_sum(name):
    """printed, not asserted: what the oracle itself changes by when the frames are summed in the opposite order"""
    x, iteration, r, _ = oracle(name)
    back = O.mcs(torch.flip(x, [1]), iteration)
    print(f"{name}: |lambda(flipped) - lambda| max {float((torch.flip(back['lam'], [1]) - r['lam']).abs().max()):.3g}")
    assert torch.equal(back["stab_adds"], r["stab_adds"])


@pytest.mark.parametrize("name", list(O.CASES))
def test_quadratic_form_identity(name):
    """trace(v v^T A^-1) / C and v^T (A^-1 / phi) v are the one form q = v^T A^-1 v.  Bound: each side rounds C^2 products of three factors and
    their sum, and once more for the division by C or phi: C^2 + 2 roundings of 2^-53 a side, relative to the sum of the terms' magnitudes
    |v|^T |A^-1| |v| (the terms cancel, so that sum and not |q| is the scale)."""
    _, _, _, trace = oracle(name)
    worst = 0.0
    for rec in trace:
        x = rec["x"]
        Cc = x.shape[-1]
        for inv, phi in zip(rec["inv"], rec["phi"]):
            q = torch.einsum("btfi,bfij,btfj->btf", x, inv, x)
            yyh = x[..., :, None] * x[..., None, :]
            tr = torch.diagonal(yyh @ inv[:, None], dim1=-2, dim2=-1).sum(-1) / Cc
            k = (x[..., None, :] @ O.safe_div(inv[:, None], phi[..., None, None]) @ x[..., None]).squeeze(-1).squeeze(-1)
            scale = torch.einsum("btfi,bfij,btfj->btf", x.abs(), inv.abs(), x.abs())
            tol = (Cc * Cc + 2) * 2.0 ** -52 * scale
            e1, e2 = (tr - q / Cc).abs() - tol / Cc, (k - O.safe_div(q, phi)).abs() - tol / torch.clamp(phi, min=1e-8)
            worst = max(worst, float(((tr - q / Cc).abs() / torch.clamp(scale, min=1e-300)).max()))
            assert float(e1.max()) <= 0 and float(e2.max()) <= 0
    print(f"{name}: |trace form - q / C| / sum|terms| max {worst:.3g}")


@pytest.mark.parametrize("name", list(O.CASES))
def test_early_stopping_stab_equals_six_steps_bit_for_bit(name):
    x, _, _, _ = oracle(name)
    xd = x.double()
    r_y = xd.permute(0, 2, 3, 1) @ xd.permute(0, 2, 1, 3) / x.shape[1]
    for r in (r_y, torch.eye(x.shape[3], dtype=torch.float64).expand(r_y.shape).clone(), torch.zeros_like(r_y)):
        full, n_full, _ = O.stab(r)
        early, n_early, _ = O.stab(r, early_stop=True)
        assert torch.equal(full.view(torch.int64), early.view(torch.int64)) and torch.equal(n_full, n_early)


@pytest.mark.parametrize("name", list(O.CASES))
def test_eigvalsh_cond_against_svdvals_cond(name):
    """both solves return every eigen/singular value to 2^-53 * C * lambda_max, so the ratio's relative error is at most 2 C 2^-53 cond: 4.4e-9
    at C = 10 under cond 1e6 * 1.25, far inside the 25 % margin.  The same additions follow."""
    x, iteration, r, trace = oracle(name)
    worst = 0.0
    xd = x.double()
    mats = [xd.permute(0, 2, 3, 1) @ xd.permute(0, 2, 1, 3) / x.shape[1]] + [a for rec in trace for a in rec["A"]]
    for m in mats:
        cs, ce = O.cond_svd(m), O.cond_eigh(m)
        near = torch.isfinite(cs) & (cs < O.EPS_INV * O.MARGIN)
        if near.any():
            rel = ((ce - cs).abs() / cs)[near]
            worst = max(worst, float(rel.max()))
            assert float((rel - 2 * x.shape[3] * 2.0 ** -53 * cs[near]).max()) <= 0
        assert torch.equal(O.stab(m, O.cond_eigh, early_stop=True)[1], O.stab(m)[1])
    print(f"{name}: |cond_eigh - cond_svd| / cond_svd max {worst:.3g}")


@pytest.mark.parametrize("name", list(O.CASES))
def test_determinant_scales(name):
    """det(phi A) = phi^C det A.  Each side is a product of C pivots of relative error at most 2^-53 cond(A), and C more roundings for the power:
    relative difference at most 2 C 2^-53 cond(A) + C 2^-52."""
    _, _, _, trace = oracle(name)
    worst = 0.0
    for rec in trace:
        Cc = rec["x"].shape[-1]
        for a, phi in zip(rec["A"], rec["phi"]):
            lit = torch.linalg.det(phi[..., None, None] * a[:, None])
            ours = phi ** Cc * torch.linalg.det(a)[:, None]
            cond = O.cond_svd(a)[:, None]
            ok = lit.abs() > 1e-290                                  # below, the product underflows on either side
            rel = ((ours - lit).abs() / lit.abs().clamp(min=1e-300))
            worst = max(worst, float(rel[ok].max()) if ok.any() else 0.0)
            assert float((rel - (2 * Cc * 2.0 ** -53 * cond + Cc * 2.0 ** -52).expand_as(rel))[ok].max() if ok.any() else 0.0) <= 0
    print(f"{name}: |phi^C det A - det(phi A)| / |det(phi A)| max {worst:.3g}")


def test_entry_points_are_in_the_header_and_the_binding(seld_lib):
    from seld_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "seld_hip.h")).read()
    assert "transforms.py:202-291" in hdr
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("seld_aug_mcs", "seld_aug_mcs_max_frames"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _lib.SIGNATURES and hasattr(seld_lib, name)
    for c in range(-1, 13):
        frames = seld_lib.seld_aug_mcs_max_frames(c)
        assert frames >= 3000 if 1 <= c <= 10 else frames == 0


def mcs_entry_point_refuses_bad_arguments(lib, p):
    """`p`: any non-NULL pointer — every call returns before anything is enqueued.  Shared with tests/test_mcs_gpu.py."""
    args = (("x", p), ("out", p), ("lam", p), ("adds", p), ("B", 1), ("T", 4), ("F", 2), ("C", 7), ("iteration", 2), ("theta", 1e-6), ("stream", None))
    call = lambda **kw: lib.seld_aug_mcs(*[kw.get(n, d) for n, d in args])
    for name in ("x", "out"):
        assert call(**{name: None}) == INVALID, name
    for name in ("B", "T", "F"):
        for bad in (0, -1):
            assert call(**{name: bad}) == INVALID, name
    for bad in (0, -3):
        assert call(iteration=bad) == INVALID
    for bad in (-1e-6, math.inf, -math.inf, math.nan):
        assert call(theta=bad) == INVALID, bad
    for bad in (0, -1, 11, 17):
        assert call(C=bad) == UNSUPPORTED, bad
    for c in range(1, 11):
        assert call(C=c, T=lib.seld_aug_mcs_max_frames(c) + 1) == UNSUPPORTED, c


def test_mcs_entry_point_refuses_bad_arguments(seld_lib):
    buf = (C.c_double * 64)()
    mcs_entry_point_refuses_bad_arguments(seld_lib, C.cast(buf, C.c_void_p))
    assert not any(buf)


def test_transforms_mcs_aug_refuses_what_the_entry_point_refuses(seld_lib):
    from seld_amd import transforms
    with pytest.raises(ValueError):
        transforms.mcs_aug(0)
    y = torch.zeros(2, 4, 8)
    with pytest.raises(ValueError):
        transforms.mcs_aug(2)(torch.zeros(2, 4, 3, 7), y)                         # a host tensor
    with pytest.raises(ValueError):
        transforms.mcs_aug(2)(torch.zeros(2, 4, 3, 11), y)                        # C = 11
    with pytest.raises(ValueError):
        transforms.mcs_aug(2)(torch.zeros(2, 4, 7, 3).transpose(2, 3), y)         # not contiguous
    with pytest.raises(ValueError):
        transforms.mcs_mask(torch.zeros(2, 4, 3, 7), 0)
    assert "mcs_aug(iteration, theta)" in transforms.__doc__ and "outside the accelerated path" not in transforms.__doc__
