"""conv_pool_sb.hip after its epilogue was re-counted in issue slots (scalar BatchNorm sums on two accumulators per channel half,
v_max3_f32, a branch-free position search, no accumulator zeroing in front of the matrix segment) must compute what it computed before: zext, amax
and the statistics of seld_k_conv_first_fwd_pool, and two seldnet train steps, against fixtures recorded ONCE from the parent commit's library
(tests/golden/make_golden_conv1_issue_budget.py, which also builds the inputs: fixed seeds, exact ties planted inside pooling windows, gamma of
both signs).  Every comparison is np.array_equal; outputs are pre-filled with NaN / 255 so an unwritten element shows."""
import importlib.util
import os

import numpy as np
import pytest

from helpers import dev

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_conv1_issue_budget", os.path.join(_HERE, "golden", "make_golden_conv1_issue_budget.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)


@pytest.fixture(scope="module")
def kernel_golden():
    return np.load(os.path.join(G.FIXTURE_DIR, "kernel.npz"))


@pytest.fixture(scope="module")
def train_golden():
    return np.load(os.path.join(G.FIXTURE_DIR, "train.npz"))


def test_inputs_hold_ties_and_both_signs():
    """what the fixtures were recorded on: ties in every case, of all three kinds, and eight or more negative channels"""
    for B, H, Cin in G.CASES:
        x, _, _, gamma, planted = G.kernel_inputs(B, H, Cin)
        assert (gamma < 0).sum() >= 8 and (gamma > 0).sum() >= 8
        assert len({(cs, cd) for *_, (_, cs), (_, cd) in planted}) == 3
        for b, k, m, (rs, cs), (rd, cd) in planted:
            ts, td = 5 * k + rs, 5 * k + rd
            assert np.array_equal(x[b, ts - 1:ts + 2, 4 * m + cs - 1:4 * m + cs + 2], x[b, td - 1:td + 2, 4 * m + cd - 1:4 * m + cd + 2])


@pytest.mark.parametrize("with_amax,with_stats", G.FORMS, ids=["training", "positions", "inference"])
@pytest.mark.parametrize("B,H,Cin", G.CASES, ids=[G.case_name(*c) for c in G.CASES])
def test_kernel_keeps_the_parent_bits(seld_lib, kernel_golden, B, H, Cin, with_amax, with_stats):
    x, w, bias, gamma, _ = G.kernel_inputs(B, H, Cin)
    ze, am, st = G.run_kernel(seld_lib, tuple(dev(a) for a in (x, w, bias, gamma)), B, H, Cin, with_amax, with_stats)
    n = G.case_name(B, H, Cin)
    want = kernel_golden[n + ".zext"]
    print(f"{n} amax={with_amax} stats={with_stats}: zext differs at {int((ze != want).sum())} of {want.size}")
    assert np.array_equal(ze, want), "zext"
    if with_amax:
        want = kernel_golden[n + (".amax" if with_stats else ".amax_nostats")]
        print(f"  amax differs at {int((am != want).sum())} of {want.size}")
        assert np.array_equal(am, want), "amax"
    else:
        assert (am == 255).all(), "amax written without being asked for"
    if with_stats:
        want = kernel_golden[n + ".stats"]
        print(f"  statistics differ at {int((st != want).sum())} of 128")
        assert np.array_equal(st, want), "statistics"
    else:
        assert np.isnan(st).all(), "statistics written without being asked for"


def test_train_steps_keep_the_parent_bits(seldnet_config, train_golden):
    """Two train steps of seldnet at B = 2, T = 50: outputs, losses, gradients, weights and BatchNorm state.  The large arrays are held to the
    recorded SHA-256 of their bytes (equal digests = equal arrays) and to a strided sample that says where they part."""
    got = G.fixture_form(G.train_items(seldnet_config))
    assert sorted(got) == sorted(train_golden.files)
    assert {"sed0", "doa1", "sloss0", "dloss1", "grad0.sha256", "grad1.sha256", "weights.sha256", "state"} <= set(got)
    for k in sorted(got):
        a, b = got[k], train_golden[k]
        print(f"{k}: differs at {int((np.asarray(a) != b).sum()) if a.shape == b.shape else 'shape'} of {b.size}")
    for k in sorted(got):
        assert np.array_equal(got[k], train_golden[k]), k
