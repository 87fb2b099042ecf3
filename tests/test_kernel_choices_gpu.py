"""Kernel choices travel as arguments (csrc/common.h KernelChoices): a context's launches read the context's, the seld_k_* entry points
read seld_k_set_option's, and neither reaches the other — whatever ran before, on this host thread or on another.  Every comparison is
bit-exact; every buffer a kernel writes starts as NaN and must come back finite."""
import threading

import numpy as np
import pytest
import torch

from helpers import dev, ptr

pytestmark = pytest.mark.gpu

B, T = 2, 50


@pytest.fixture(scope="module")
def batch(seldnet_config):
    """The weights and the batch every step of this module starts from (read-only)."""
    from oracle import seldnet_oracle as O
    w, st = O.random_weights(O.Spec.from_config(seldnet_config), 0)
    return (w, st) + tuple(O.synthetic_batch(B, T))


def _context(seldnet_config, options=()):
    from seld_amd import models
    model = models.seldnet((B, T, 64, 7), seldnet_config)
    for key, value in dict(options).items():
        model.set_option(key, value)
    return model


def _step_grads(model, batch):
    """One training step from the module's weights and dropout step counter 0 -> the gradients it left (which started as NaN)."""
    from seld_amd import losses, train
    w, st, x, ys, yd = batch
    model.set_weights(w, st)
    model.set_option("dropout_step", 0)
    model.grad_tensor().fill_(float("nan"))
    y_p, sl, dl = train.trainstep(model, x, (ys, yd), losses.BinaryCrossentropy(), losses.MSE, (1.0, 1000.0), train.Adam(1e-3))
    g = model.get_grads().copy()
    for a in (g, y_p[0].cpu().numpy(), y_p[1].cpu().numpy(), sl.cpu().numpy(), dl.cpu().numpy()):
        assert np.isfinite(a).all()
    assert np.abs(g).max() > 0
    return g


SINGLE_SIX = {"bf16_single": 1, "bwd_four_products": 0}       # what a default context is not: one product forward, no four-product backward


def test_a_contexts_choices_do_not_reach_the_kernel_entry_points(seld_lib, seldnet_config, batch):
    """seld_k_gemm_sb (M = 33, N = 128, K = 128, mode 0), seld_k_conv3x3_dgrad (B = 1, H = 3, W = 4) and seld_k_gemm_tn (M = 64, K1 = 128,
    N = 128) — launchers that branch on the single-product, four-product and tile-block choices — give the same bits before and after a
    context with bf16_single = 1, bwd_four_products = 0, dgrad_r8 = 0, tn_tile_blocks = 64 has run a training step."""
    rng = np.random.default_rng(71)
    A = dev(rng.standard_normal((33, 128)))
    Bm = dev(rng.standard_normal((128, 128)) / np.sqrt(128))
    bias = dev(rng.standard_normal(128))
    dz = dev(rng.standard_normal((1, 3, 4, 64)))
    w = dev(rng.standard_normal((3, 3, 64, 64)) / 24)
    At, Bt = dev(rng.standard_normal((64, 128))), dev(rng.standard_normal((64, 128)))

    def entry_points():
        nan = lambda *shape: torch.full(shape, float("nan"), device="cuda")
        C0, dx, Ct, cs = nan(33, 128), nan(1, 3, 4, 64), nan(128, 128), nan(128)
        assert seld_lib.seld_k_gemm_sb(ptr(A), None, ptr(Bm), None, ptr(bias), None, ptr(C0), None, 33, 128, 128, 0, 0, 0) == 0
        assert seld_lib.seld_k_conv3x3_dgrad(ptr(dz), ptr(w), ptr(dx), 1, 3, 4, 64, 64) == 0
        assert seld_lib.seld_k_gemm_tn(ptr(At), ptr(Bt), ptr(Ct), ptr(cs), 64, 128, 128) == 0
        out = [t.cpu().numpy() for t in (C0, dx, Ct, cs)]
        for a in out:
            assert np.isfinite(a).all()
        return out

    before = entry_points()
    model = _context(seldnet_config, {**SINGLE_SIX, "dgrad_r8": 0, "tn_tile_blocks": 64})
    _step_grads(model, batch)
    after = entry_points()
    model.close()
    for a, b in zip(before, after):
        np.testing.assert_array_equal(a, b)


def test_the_retired_conv64_dbuf_key_is_refused(seld_lib, seldnet_config):
    """"conv64_dbuf" chose between two region kernels of conv_sb.hip; one of them is gone and so is the key: a context's set_option and
    seld_k_set_option refuse it like any unknown key, and still take the keys that stayed."""
    from seld_amd import _lib
    model = _context(seldnet_config)
    try:
        with pytest.raises(_lib.SeldError) as e:
            model.set_option("conv64_dbuf", 1)
        assert e.value.code != 0
        assert seld_lib.seld_set_option(model.ctx, b"conv64_dbuf", 0) != 0
        model.set_option("dgrad_r8", 1)
        model.set_option("bwd_four_products", 1)
    finally:
        model.close()
    assert seld_lib.seld_k_set_option(b"conv64_dbuf", 1) != 0
    assert seld_lib.seld_k_set_option(b"conv64_dbuf", 0) != 0
    assert seld_lib.seld_k_set_option(b"bwd_four_products", 1) == 0
    assert seld_lib.seld_k_set_option(b"dgrad_r8", 1) == 0              # the entry points' own copy of the key (its default)


def test_kernel_entry_point_options_do_not_reach_a_context(seld_lib, seldnet_config, batch):
    """A default context's gradients are the same bits with seld_k_set_option's bf16_single = 1, bwd_four_products = 0, gsb_dbg = 4 set."""
    model = _context(seldnet_config)
    g = _step_grads(model, batch)
    try:
        for key, value in ((b"bf16_single", 1), (b"bwd_four_products", 0), (b"gsb_dbg", 4)):
            assert seld_lib.seld_k_set_option(key, value) == 0
        g_set = _step_grads(model, batch)
    finally:
        for key, value in ((b"bf16_single", 0), (b"bwd_four_products", 1), (b"gsb_dbg", 0)):
            seld_lib.seld_k_set_option(key, value)
    model.close()
    np.testing.assert_array_equal(g_set, g)


def test_two_contexts_with_different_choices_do_not_disturb_each_other(seldnet_config, batch):
    """Context A (defaults) and context B (bf16_single = 1, bwd_four_products = 0): each one's gradients of a step run alone are what it
    computes after the other has run, and while the other runs on a second host thread (three steps each, started together)."""
    ctx = [_context(seldnet_config), _context(seldnet_config, SINGLE_SIX)]
    solo = [_step_grads(m, batch) for m in ctx]
    assert not np.array_equal(solo[0], solo[1])                 # the two choices do differ in their bits
    _step_grads(ctx[1], batch)
    np.testing.assert_array_equal(_step_grads(ctx[0], batch), solo[0])

    start = threading.Barrier(2)
    got, errors = [[], []], []

    def run(r):
        try:
            with torch.cuda.stream(torch.cuda.Stream()):
                start.wait(timeout=60)
                for _ in range(3):
                    got[r].append(_step_grads(ctx[r], batch))
        except Exception as e:           # noqa: BLE001
            errors.append(e)
            start.abort()

    ths = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    for th in ths:
        th.start()
    for th in ths:
        th.join(timeout=120)
        assert not th.is_alive()
    assert not errors, errors
    for r in range(2):
        assert len(got[r]) == 3
        for g in got[r]:
            np.testing.assert_array_equal(g, solo[r])
    for m in ctx:
        m.close()
