"""seld_aug_mcs / transforms.mcs_aug on the device against the literal float64 oracle (tests/mcs_oracle.py), case by case: the stab decisions
exactly, the mask to a derived ceiling, the product to fp32 rounding; then the bit-level contracts of the entry point."""
import ctypes as C

import pytest
import torch

import mcs_oracle as O
from helpers import rel_err
from test_mcs_cpu import mcs_entry_point_refuses_bad_arguments, oracle

pytestmark = pytest.mark.gpu

# |lambda_dev - lambda_oracle|: backward-stable solves on matrices the decision rule keeps under cond 1e6 give
# 2.2e-16 * 1e6 * C^2 * (iteration + 1) <= 9e-8 at C = 10, iteration 3 (a ceiling, not a measurement)
LAMBDA_TOL = 1e-7
# out against float32(x) * float32(lambda_oracle), tensor-normalised: two fp32 roundings (1.2e-7) plus the ceiling above
OUT_TOL = 1e-6


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def run(lib, x, iteration, theta=1e-6, in_place=False, want_lambda=True, want_adds=True):
    """x: a device tensor, left alone unless in_place -> (out, lambda or None, stab_adds or None)"""
    B, T, F, Cc = x.shape
    out = x if in_place else torch.full_like(x, float("nan"))
    lam = torch.full((B, T, F), float("nan"), dtype=torch.float64, device="cuda") if want_lambda else None
    adds = torch.full((B, F, 2, iteration + 1), -1, dtype=torch.int32, device="cuda") if want_adds else None
    rc = lib.seld_aug_mcs(ptr(x), ptr(out), ptr(lam), ptr(adds), B, T, F, Cc, iteration, theta, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    return out, lam, adds


@pytest.mark.parametrize("name", list(O.CASES))
def test_against_the_literal_oracle(seld_lib, name):
    x, iteration, ref, _ = oracle(name)
    out, lam, adds = run(seld_lib, x.cuda(), iteration)
    adds, lam, out = adds.cpu(), lam.cpu(), out.cpu()
    differ = int((adds != ref["stab_adds"]).sum())
    print(f"{name}: stab_adds that differ {differ} of {adds.numel()}; additions seen {sorted(set(adds.flatten().tolist()))}")
    assert differ == 0
    err = float((lam - ref["lam"]).abs().max())
    print(f"{name}: |lambda_dev - lambda_oracle| max {err:.3g} (ceiling {LAMBDA_TOL:g})")
    assert err <= LAMBDA_TOL
    want = x * ref["lam"][..., None].float()
    e_out = rel_err(out.numpy(), want.numpy())
    print(f"{name}: out against float32(x) * float32(lambda_oracle), tensor-normalised {e_out:.3g} (bound {OUT_TOL:g})")
    assert e_out <= OUT_TOL
    assert torch.equal(out, x * lam[..., None].float())      # the product is the fp32 one of the device's own mask


@pytest.mark.parametrize("name", ["past_a_wave", "masked", "past_256_widest"])
def test_bits_in_place_repeated_and_without_optional_outputs(seld_lib, name):
    x, iteration, _, _ = oracle(name)
    xd = x.cuda()
    out, lam, adds = run(seld_lib, xd, iteration)
    assert torch.equal(xd.cpu(), x)                                             # out of place leaves x alone
    again = run(seld_lib, xd, iteration)
    for a, b in zip((out, lam, adds), again):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))            # two calls, the same bits
    bare, _, _ = run(seld_lib, xd, iteration, want_lambda=False, want_adds=False)
    assert torch.equal(bare.view(torch.int32), out.view(torch.int32))
    inplace = xd.clone()
    run(seld_lib, inplace, iteration, in_place=True)
    assert torch.equal(inplace.view(torch.int32), out.view(torch.int32))


def test_mcs_aug_runs_the_reference_test(seld_lib):
    """transforms_test.py:97-102: x [3,7,4,2], y [3,7,14], mcs_aug(2); shapes kept, y returned as it is"""
    from seld_amd import transforms
    x, iteration, ref, _ = oracle("reference_test")
    xd, y = x.cuda(), torch.rand(3, 7, 14, device="cuda")
    x2, y2 = transforms.mcs_aug(iteration)(xd, y)
    torch.cuda.synchronize()
    assert x2 is xd and y2 is y and x2.shape == x.shape and y2.shape == (3, 7, 14)
    e = rel_err(x2.cpu().numpy(), (x * ref["lam"][..., None].float()).numpy())
    print(f"mcs_aug(2) on the reference's test: tensor-normalised {e:.3g}")
    assert e <= OUT_TOL


def test_mcs_mask_leaves_x_unchanged(seld_lib):
    from seld_amd import transforms
    x, iteration, ref, _ = oracle("past_a_wave")
    xd = x.cuda()
    lam, adds = transforms.mcs_mask(xd, iteration)
    torch.cuda.synchronize()
    assert torch.equal(xd.cpu(), x)
    assert lam.dtype == torch.float64 and lam.shape == x.shape[:3] and adds.dtype == torch.int32
    assert torch.equal(adds.cpu(), ref["stab_adds"]) and float((lam.cpu() - ref["lam"]).abs().max()) <= LAMBDA_TOL


def test_refusals_with_device_pointers(seld_lib):
    from seld_amd import transforms
    buf = torch.zeros(64, dtype=torch.float64, device="cuda")
    mcs_entry_point_refuses_bad_arguments(seld_lib, ptr(buf))
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0      # nothing was enqueued
    y = torch.zeros(2, 4, 8, device="cuda")
    with pytest.raises(ValueError):
        transforms.mcs_aug(2)(torch.zeros(2, 4, 3, 11, device="cuda"), y)
    with pytest.raises(ValueError):
        transforms.mcs_aug(2)(torch.zeros(2, 4, 7, 3, device="cuda").transpose(2, 3), y)
    with pytest.raises(ValueError):
        transforms.mcs_aug(2)(torch.zeros(1, seld_lib.seld_aug_mcs_max_frames(7) + 1, 1, 7, device="cuda"), y)
    with pytest.raises(ValueError):
        transforms.mcs_aug(2, theta=-1.0)(torch.zeros(2, 4, 3, 7, device="cuda"), y)
