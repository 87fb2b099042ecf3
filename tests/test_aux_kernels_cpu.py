"""What tests/test_aux_kernels_gpu.py rests on, checked without a GPU: the conditions its metrics cases must meet, that its bars can be met by a
plain fp32 evaluation, that the numpy references of tests/aux_kernel_cases.py agree with oracle/, and every refusal of the entry points of
metrics.hip, infer.hip, augment.hip and feat_stats.hip (each validates its arguments before its first HIP call, so dummy pointers are never
dereferenced and no device is needed)."""
import numpy as np
import pytest

import aux_kernel_cases as A
from oracle import features_oracle as FO
from oracle import infer_oracle as IO
from oracle import transforms_oracle as TO

OK, INVALID, UNSUPPORTED = 0, -1, -2
P = 0x1000          # a non-null pointer that is never dereferenced

ALL_METRICS = A.METRICS_CASES
metrics_cases = pytest.mark.parametrize("case", ALL_METRICS, ids=A.metrics_id)


# ---------------------------------------------------------------- metrics: the cases and their bars
@metrics_cases
def test_restatement_in_fp64_is_the_oracle(case):
    """the restated update_block_states, in float64, gives the oracle's state bit for bit: the margins are the oracle's own intermediate values"""
    ref, _, _ = A.metrics_reference(case)
    got, _ = A.restated_metrics([A.metrics_inputs(case)], case.nc, case.block, np.float64)
    A.report_exact(f"restated fp64 {A.metrics_id(case)}", got, ref)


@metrics_cases
def test_metrics_case_conditions(case):
    """Conditions on the committed seeds: threshold margin >= 1e-3 deg, no sed_pred at 0.5, DE_TP > 0, and for the noise = 0.25 cases an item on
    each side of the threshold (a case of one item cannot have both: the condition holds from two items on)."""
    m = A.metrics_margins(case)
    print(f"[parity] conditions {A.metrics_id(case):40s} {m}")
    assert m.threshold >= 1e-3
    assert m.sed > 0 and m.n_half == 0
    assert m.de_tp > 0
    if case.noise == 0.25 and case.B * A.n_blocks(case.S, case.block) * case.nc > 1:
        assert m.n_close > 0 and m.n_far > 0
    ref, _, _ = A.metrics_reference(case)
    assert ref[A.IDX_DE_TP] == m.de_tp


@metrics_cases
def test_bars_can_be_met_in_fp32(case):
    """A plain float32 evaluation equals the fp64 oracle on every counter, is within de_bar on total_DE, and de_bar stays a small part of DE_TP."""
    ref, _, _ = A.metrics_reference(case)
    m = A.metrics_margins(case)
    got, _ = A.restated_metrics([A.metrics_inputs(case)], case.nc, case.block, np.float32)
    keep = np.arange(ref.size) != A.IDX_TOTAL_DE
    A.report_exact(f"fp32 counters {A.metrics_id(case)}", got[keep], ref[keep])
    A.report(f"fp32 total_DE {A.metrics_id(case)}", abs(got[A.IDX_TOTAL_DE] - ref[A.IDX_TOTAL_DE]), m.de_bar)
    A.report(f"de_bar / DE_TP {A.metrics_id(case)}", m.de_bar, 0.05 * m.de_tp)


def test_case_table_geometries():
    got = {(c.B, c.S, c.nc, c.block, c.noise) for c in ALL_METRICS}
    assert got == {(1, 1, 1, 1, 0.25), (3, 25, 12, 10, 0.25), (5, 7, 3, 4, 0.25), (2, 33, 13, 1, 0.25), (2, 64, 14, 32, 0.25),
                   (30, 95, 12, 10, 0.25), (30, 95, 12, 10, 1e-3), (256, 60, 12, 10, 0.25)}
    items = [c.B * A.n_blocks(c.S, c.block) for c in ALL_METRICS]
    assert max(items) == 1536 and 300 in items          # past the items kernel's 128 and the reduce kernel's 256


def test_tile_classes():
    rng = np.random.default_rng(0)
    sed, doa = rng.random((2, 3, 12)), rng.random((2, 3, 36))
    s, d = A.tile_classes(sed, doa, 14)
    assert s.shape == (2, 3, 14) and d.shape == (2, 3, 42)
    np.testing.assert_array_equal(s[..., 12:], sed[..., :2])
    for k in range(3):
        np.testing.assert_array_equal(d[..., 14 * k:14 * k + 12], doa[..., 12 * k:12 * k + 12])
        np.testing.assert_array_equal(d[..., 14 * k + 12:14 * k + 14], doa[..., 12 * k:12 * k + 2])
    s, d = A.tile_classes(sed, doa, 3)
    np.testing.assert_array_equal(d, np.concatenate([doa[..., 12 * k:12 * k + 3] for k in range(3)], -1))


def test_hand_built_case_is_what_it_says():
    """the fp64 oracle on the hand-built tensors gives the counters worked by hand, in fp32 as well; the special elements are where they should be"""
    c = A.HAND
    upd = [A.hand_built_inputs()]
    om = A.oracle_metrics(upd, c.nc, c.block)
    for k, v in A.HAND_EXPECTED.items():
        np.testing.assert_array_equal(getattr(om, k), v, err_msg=k)
    m = A.margins(upd, c.nc, c.block)
    assert m.n_half == 1 and m.n_close == 3 and m.n_far == 1 and m.threshold > 0.99
    assert abs(om.total_DE - 40.0) < 1e-4                   # 19 + 21 + 0 + 0: the (1,-1,0) / (0,1,-1) pair counts as 0, not 120
    got, _ = A.restated_metrics(upd, c.nc, c.block, np.float32)
    ref = om.state_vector()
    keep = np.arange(ref.size) != A.IDX_TOTAL_DE
    A.report_exact("hand-built fp32 counters", got[keep], ref[keep])
    A.report("hand-built fp32 total_DE", abs(got[A.IDX_TOTAL_DE] - ref[A.IDX_TOTAL_DE]), m.de_bar)
    sed_t, doa_t, sed_p, doa_p = upd[0]
    a, q = doa_t[0, 11].reshape(3, 4)[:, 1], doa_p[0, 11].reshape(3, 4)[:, 1]
    assert a.sum() == 0 and q.sum() == 0 and a.dtype == np.float32


def test_angle_allowance():
    """e(theta) is largest at theta = 0, where arccos is ill-conditioned: sqrt(2 delta) rad = 0.04 deg; 4e-5 deg at the threshold"""
    e = A.angle_allowance(np.array([0.0, 0.06, 20.0, 90.0, 180.0]))
    assert abs(e[0] - np.rad2deg(np.sqrt(2 * A.DELTA))) < 1e-6
    assert (np.diff(e[:4]) < 0).all() and e[4] == 0
    assert 3e-5 < e[2] < 5e-5


# ---------------------------------------------------------------- the other references against oracle/
@pytest.mark.parametrize("shape", A.OVERLAP_CASES, ids=str)
def test_overlap_window_index_reference(shape):
    n_win, L, _ = shape
    y, want = A.overlap_window_index_inputs(n_win, L)
    np.testing.assert_array_equal(IO.overlap_average(y.astype(np.float64)), want)


@pytest.mark.parametrize("shape", A.MASK_CASES, ids=str)
def test_mask_reference_and_draws(shape):
    """the numpy mask of both axes in one call equals oracle.transforms_oracle.mask applied axis by axis; the draws hold the edge cases"""
    B, T, F, C, period = shape
    x, sets = A.mask_inputs(*shape)
    nseg = T // period
    cat = [np.concatenate([s[i] for s in sets]) for i in range(4)]
    for off, size, total in ((cat[0], cat[1], period), (cat[2], cat[3], F)):
        assert ((size == 0) & (off > 0)).any()
        assert ((off + size == total) & (size > 0) & (size < total)).any()
        assert ((off == 0) & (size == total)).any()
    for t_off, t_size, f_off, f_size in sets:
        assert t_off.dtype == np.int32 and t_off.shape == (B * nseg,)
        both = A.mask_reference(x, period, t_off, t_size, f_off, f_size)
        for b in range(B):
            sl = slice(b * nseg, (b + 1) * nseg)
            ref_t = TO.mask(x[b], -3, t_size[sl], t_off[sl], period)
            np.testing.assert_array_equal(A.mask_reference(x, period, t_off, t_size)[b], ref_t)
            np.testing.assert_array_equal(both[b], TO.mask(ref_t, -2, f_size[sl], f_off[sl], period))
        assert (both == 0).any() and (x != 0).all()


def test_gather_sign_reference():
    """the numpy gather / sign against the explicit loop of the header's statement, and against foa_intensity_vec_aug's intensity-vector shuffle"""
    x, src, sgn = A.gather_inputs(3, 5, 4, 12, "repeats")
    want = np.empty_like(x)
    for b in range(3):
        for r in range(4):
            want[b, :, r] = sgn[b, r] * x[b, :, src[b, r]]
    np.testing.assert_array_equal(A.gather_sign_reference(x, src, sgn), want)
    rng = np.random.default_rng(5)
    xx = rng.standard_normal((4, 6, 5, 7)).astype(np.float32)
    flip, p = rng.integers(0, 2, (4, 3)), 2 * rng.integers(0, 2, 4)
    xo, _ = TO.foa_intensity_vec_aug(xx, np.zeros((4, 2, 8), np.float32), flip, p)
    perm = np.stack([p, np.ones_like(p), 2 - p], -1)
    feat_perm = (perm + (perm != np.arange(3)).sum(-1, keepdims=True)) % 3
    iv = A.gather_sign_reference(xx[..., 4:].reshape(4, 30, 3, 1), feat_perm, (1 - 2 * np.take_along_axis(flip, feat_perm, 1)).astype(np.float32))
    np.testing.assert_array_equal(iv.reshape(4, 6, 5, 3), xo[..., 4:])
    for shape in A.GATHER_CASES:
        _, s, g = A.gather_inputs(*shape, "permutation")
        assert (np.sort(s, 1) == np.arange(shape[2])).all() and set(np.unique(g)) <= {-1.0, 1.0}
    _, s, _ = A.gather_inputs(2, 300, 17, 1, "repeats")
    assert any(len(set(row)) < 17 for row in s)


def test_frame_reference_on_index_input():
    T, FC, win, step, first, n = A.FRAME_CASES[1]
    w = IO.frame(A.frame_inputs(T, FC, "index"), win, step)[first:first + n]
    assert w.shape == (n, win, FC) and w[0, 0, 0] == first * step * FC and w[-1, -1, -1] == T * FC - 1 - ((T - win) % step) * FC


def test_stats_reference():
    x = A.stats_inputs(17, 448)
    m, s, mean_bar, std_bar = A.stats_reference(x)
    rm, rs = FO.calculate_statistics([x[:9].astype(np.float64), x[9:].astype(np.float64)])
    np.testing.assert_allclose(m, rm[0], rtol=1e-14)
    np.testing.assert_allclose(s, rs[0], rtol=1e-12)
    big = A.stats_inputs(8200, 257)
    s_big = big.astype(np.float64).std(0)
    assert s_big.min() < 2e-3 and s_big.max() > 50 and np.abs(big).max() > 100
    (em, bm), (es, bs) = A.stats_errors(m.astype(np.float32), s.astype(np.float32), (m, s, mean_bar, std_bar))
    assert em <= bm and es <= bs                        # the reference itself, rounded to float32, meets its bars
    one = A.stats_reference(A.stats_inputs(1, 1))
    assert one[1][0] == 0 and one[3][0] == 0
    assert A.stats_errors(one[0], [0.0], one) == ((0.0, one[2][0]), (0.0, 0.0))
    assert A.stats_errors(one[0], [1e-30], one)[1][0] > 0


# ---------------------------------------------------------------- refusals, before any HIP call
def _metrics_args(**kw):
    a = dict(sed_true=P, doa_true=P, sed_pred=P, doa_pred=P, B=2, S=20, nc=4, block=10, thr=20.0, state=P, scratch=P)
    a.update(kw)
    return [a[k] for k in ("sed_true", "doa_true", "sed_pred", "doa_pred", "B", "S", "nc", "block", "thr", "state", "scratch")] + [None]


def test_metrics_update_refusals(seld_lib):
    for name in ("sed_true", "doa_true", "sed_pred", "doa_pred", "state", "scratch"):
        assert seld_lib.seld_metrics_update(*_metrics_args(**{name: None})) == INVALID, name
    for name in ("B", "S", "nc", "block"):
        for v in (0, -1):
            assert seld_lib.seld_metrics_update(*_metrics_args(**{name: v})) == INVALID, (name, v)
    assert seld_lib.seld_metrics_update(*_metrics_args(block=33)) == INVALID


def test_metrics_sizes(seld_lib):
    assert seld_lib.seld_metrics_scratch_floats(2, 20, 4, 0) == -1
    for c in ALL_METRICS + (A.HAND,):
        assert seld_lib.seld_metrics_state_size(c.nc) == 11 + 4 * c.nc == A.state_size(c.nc)
        assert seld_lib.seld_metrics_scratch_floats(c.B, c.S, c.nc, c.block) == c.B * -(-c.S // c.block) * (11 + 4 * c.nc)


def test_frame_windows_refusals(seld_lib):
    f = seld_lib.seld_frame_windows                     # (x, windows, T, FC, win, step, first, n, stream)
    assert f(P, P, 23, 6, 5, 3, 0, 7, None) == INVALID                  # FC % 4 != 0
    assert f(P, P, 23, 4, 5, 3, -1, 7, None) == INVALID                 # first_window < 0
    assert f(P, P, 23, 4, 5, 3, 0, 0, None) == INVALID                  # n_windows = 0
    assert f(P, P, 22, 4, 5, 3, 0, 7, None) == INVALID                  # the last window covers frames 18..22: one past T = 22
    assert f(P, P, 25, 4, 5, 3, 2, 6, None) == INVALID                  # the same through first_window: frames 21..25 of T = 25
    assert f(None, P, 23, 4, 5, 3, 0, 7, None) == INVALID and f(P, None, 23, 4, 5, 3, 0, 7, None) == INVALID
    # (23, 4, 5, 3, 0, 7) ends exactly at T and is accepted: it launches, so tests/test_aux_kernels_gpu.py runs it


def test_overlap_average_refusals(seld_lib):
    f = seld_lib.seld_overlap_average                   # (y, out, n_windows, L, D, stream)
    assert f(None, P, 3, 4, 5, None) == INVALID and f(P, None, 3, 4, 5, None) == INVALID
    for bad in (0, -1):
        assert f(P, P, bad, 4, 5, None) == INVALID
        assert f(P, P, 3, bad, 5, None) == INVALID
        assert f(P, P, 3, 4, bad, None) == INVALID


def test_aug_mask_refusals(seld_lib):
    f = seld_lib.seld_aug_mask                          # (x, B, T, F, C, period, t_off, t_size, f_off, f_size, stream)
    assert f(P, 2, 25, 8, 7, 10, P, P, None, None, None) == INVALID     # T % period != 0
    assert f(P, 2, 20, 8, 7, 10, P, None, None, None, None) == INVALID  # offset without size, time
    assert f(P, 2, 20, 8, 7, 10, None, None, P, None, None) == INVALID  # offset without size, frequency
    assert f(P, 2, 20, 8, 7, 10, None, P, None, None, None) == INVALID  # size without offset
    assert f(P, 2, 20, 8, 7, 10, P, P, P, None, None) == INVALID
    assert f(None, 2, 20, 8, 7, 10, P, P, P, P, None) == INVALID
    assert f(P, 2, 20, 8, 7, 10, None, None, None, None, None) == OK    # nothing to mask


def test_aug_gather_sign_refusals(seld_lib):
    f = seld_lib.seld_aug_gather_sign                   # (x, B, outer, R, inner, src, sgn, stream)
    assert f(P, 2, 3, 33, 5, P, P, None) == UNSUPPORTED
    assert f(P, 2, 3, 0, 5, P, P, None) == INVALID
    assert f(P, 2, 3, 4, 5, None, P, None) == INVALID and f(P, 2, 3, 4, 5, P, None, None) == INVALID
    assert f(None, 2, 3, 4, 5, P, P, None) == INVALID
    assert f(P, 0, 3, 4, 5, P, P, None) == INVALID and f(P, 2, 0, 4, 5, P, P, None) == INVALID and f(P, 2, 3, 4, 0, P, P, None) == INVALID


def test_feat_stats_refusals(seld_lib):
    f = seld_lib.seld_feat_stats_accumulate             # (feat, rows, FC, acc, scratch, stream)
    assert f(P, 0, 448, P, P, None) == OK               # an empty file adds nothing
    assert f(P, -1, 448, P, P, None) == INVALID
    assert f(P, 5, 0, P, P, None) == INVALID
    assert f(None, 5, 448, P, P, None) == INVALID and f(P, 5, 448, None, P, None) == INVALID and f(P, 5, 448, P, None, None) == INVALID
    assert seld_lib.seld_feat_stats_scratch_doubles(0) == -1
    assert seld_lib.seld_feat_stats_scratch_doubles(257) == 512 * 2 * 257
    g = seld_lib.seld_feat_stats_finalize               # (acc, FC, mean, std, stream)
    assert g(None, 4, P, P, None) == INVALID and g(P, 4, None, P, None) == INVALID and g(P, 4, P, None, None) == INVALID and g(P, 0, P, P, None) == INVALID
