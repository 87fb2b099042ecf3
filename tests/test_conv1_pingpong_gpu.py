"""conv_pool_sb.hip, option `conv1_pingpong`: the 8-wave ping-pong form of the z-free first-block forward (Cin = 7) claims the SAME BITS as the
4-wave kernel — group g of block b plays virtual workgroup v of the 4-wave grid (csrc/conv1_pp_sched.h).  Every comparison here is torch.equal /
np.array_equal between option 0 and option 1; outputs are pre-filled with NaN / 255 so an unwritten element shows."""
import os
import re

import numpy as np
import pytest
import torch

from helpers import dev, ptr

pytestmark = pytest.mark.gpu

# (B, H): what the shape exercises (tiles = B * ceil(H / 10); 512 virtual workgroups at most)
SHAPES = [(1, 5),       # one tile, second pooling row dead, the second wave group idle
          (1, 10),      # one full tile
          (1, 15),      # two tiles, one per group, the second half-live
          (3, 25),      # 9 tiles: odd virtual grid, one block with an idle group
          (3, 1730),    # 519 tiles: streams of 2 and 1 tiles inside one block
          (4, 2600)]    # 1 040 tiles: streams of 3 and 2
CASES = [(B, H, 0) for B, H in SHAPES] + [(3, 25, 1), (3, 1730, 1)]


def _default():
    """KernelChoices::conv1_pingpong as csrc/common.h initialises it: what the process-wide seld_k_* choices go back to after a run"""
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "seld_amd", "csrc", "common.h")) as f:
        return int(re.search(r"int conv1_pingpong = (\d+);", f.read()).group(1))


def _inputs(B, H, Cin):
    rng = np.random.default_rng(11)
    x = rng.standard_normal((B, H, 64, Cin)).astype(np.float32)
    w = (rng.standard_normal((3, 3, Cin, 64)) / np.sqrt(9 * Cin)).astype(np.float32)
    b = rng.standard_normal(64).astype(np.float32)
    gamma = (rng.uniform(0.5, 1.5, 64) * np.where(rng.random(64) < 0.3, -1, 1)).astype(np.float32)
    gamma[5] = 0.0
    assert (gamma < 0).any()
    return dev(x), dev(w), dev(b), dev(gamma)


def _run(lib, pingpong, single, xd, wd, bd, gd, B, H, Cin, with_amax, with_stats):
    ze = torch.full((B, H // 5, 16, 64), float("nan"), device="cuda")
    am = torch.full((B, H // 5, 16, 64), 255, device="cuda", dtype=torch.uint8)
    st = torch.full((128,), float("nan"), device="cuda")
    assert lib.seld_k_set_option(b"conv1_pingpong", pingpong) == 0
    assert lib.seld_k_set_option(b"bf16_single", single) == 0
    try:
        rc = lib.seld_k_conv_first_fwd_pool(ptr(xd), ptr(wd), ptr(bd), ptr(gd), None, ptr(ze), ptr(am) if with_amax else None,
                                            ptr(st) if with_stats else None, B, H, Cin)
        torch.cuda.synchronize()
    finally:
        lib.seld_k_set_option(b"conv1_pingpong", _default())
        lib.seld_k_set_option(b"bf16_single", 0)
    assert rc == 0
    return ze, am, st


def _compare(lib, B, H, Cin, single):
    args = _inputs(B, H, Cin)
    # training (amax + statistics), amax without statistics, neither (inference)
    for with_amax, with_stats in ((True, True), (True, False), (False, False)):
        ze0, am0, st0 = _run(lib, 0, single, *args, B, H, Cin, with_amax, with_stats)
        ze1, am1, st1 = _run(lib, 1, single, *args, B, H, Cin, with_amax, with_stats)
        form = f"{(B, H, Cin)} single={single} amax={with_amax} stats={with_stats}"
        assert not torch.isnan(ze0).any(), form
        assert torch.equal(ze0, ze1), f"zext differs: {form}"
        if with_amax:
            assert am0.max().item() < 20, form
            assert torch.equal(am0, am1), f"amax differs: {form}"
        else:
            assert (am1 == 255).all(), f"amax written without being asked for: {form}"
        if with_stats:
            assert not torch.isnan(st0).any(), form
            assert torch.equal(st0, st1), f"statistics differ: {form}"


@pytest.mark.parametrize("B,H,single", CASES)
def test_pingpong_kernel_is_bit_identical(seld_lib, B, H, single):
    _compare(seld_lib, B, H, 7, single)


def test_pingpong_cin10_keeps_the_four_wave_kernel(seld_lib):
    """Two patches of 16 channel slots do not fit the LDS: with the option on, Cin = 10 runs the 4-wave kernel — the same bits."""
    _compare(seld_lib, 3, 25, 10, 0)


def test_pingpong_train_steps_are_bit_identical(seldnet_config):
    """Two train steps of seldnet on [2, 100, 64, 7] from the same seed with the option 0 and 1: outputs, losses, gradients, weights and BatchNorm
    state bit for bit (the pattern of test_folded_passes_are_bit_identical_to_the_stand_alone_ones)."""
    from oracle import seldnet_oracle as O
    from seld_amd import losses, models, train
    B, T = 2, 100

    def run(value):
        spec = O.Spec.from_config(seldnet_config)
        w, st = O.random_weights(spec, 0)
        x, ys, yd = O.synthetic_batch(B, T, seed=1234)
        model = models.seldnet((B, T, 64, 7), seldnet_config)
        model.set_weights(w, st)
        model.set_option("conv1_pingpong", value)
        got = []
        opt_ = train.Adam(1e-3)
        for _ in range(2):
            y_p, sl, dl = train.trainstep(model, x, (ys, yd), losses.BinaryCrossentropy(), losses.MMSE, (1.0, 1000.0), opt_)
            got += [y_p[0].cpu().numpy().copy(), y_p[1].cpu().numpy().copy(), sl.cpu().numpy().copy(), dl.cpu().numpy().copy(), model.get_grads().copy()]
        got += list(model.get_weights())
        model.close()
        return got

    ref, alt = run(0), run(1)
    assert len(ref) == len(alt) == 12
    for i, (a, b) in enumerate(zip(ref, alt)):
        assert np.isfinite(a).all(), f"item {i}"
        assert np.array_equal(a, b), f"item {i} differs: max |d| = {np.abs(a.astype(np.float64) - b).max():.3e}"
