"""The small kernels around the train step, each called through the C ABI and compared with a plain fp64 numpy reference at the sizes where
its code takes another path: metrics.hip (up to twelve thread blocks of the items kernel, the reduce kernel's stride), infer.hip
(window indices, the 8-wide unrolled sum and its tail), augment.hip (both mask axes in one call, R up to the register-array limit) and
feat_stats.hip (the 512-chunk cap, empty trailing chunks, several columns per thread).  Cases, inputs, references and the reasoning behind
every bar are in tests/aux_kernel_cases.py; tests/test_aux_kernels_cpu.py holds the conditions the cases meet.  Every output buffer starts
as NaN (an accumulator as zero), and buffers next to the written range carry NaN guard rows that must stay NaN."""
import ctypes as C

import numpy as np
import pytest
import torch

import aux_kernel_cases as A
import helpers
from helpers import ptr
from oracle import infer_oracle as IO

pytestmark = pytest.mark.gpu

OK, UNSUPPORTED = 0, -2
NAN = float("nan")


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(a):
    return helpers.dev(np.array(a))          # a copy: the shared inputs are read-only, which torch does not take


def idev(a):
    return torch.as_tensor(np.array(a, np.int32)).cuda()


def nans(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device="cuda")


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


# ---------------------------------------------------------------- metrics
def direct_update(lib, state, upd, nc, block, thr=A.DOA_THRESHOLD):
    """seld_metrics_update on contiguous device copies, with a scratch buffer of exactly the advertised size, preset to NaN, and a guard"""
    sed_t, doa_t, sed_p, doa_p = (dev(a) for a in upd)
    B, S, _ = sed_t.shape
    need = lib.seld_metrics_scratch_floats(B, S, nc, block)
    scratch = nans(need + 64)
    assert lib.seld_metrics_update(ptr(sed_t), ptr(doa_t), ptr(sed_p), ptr(doa_p), B, S, nc, block, thr, ptr(state), ptr(scratch), stream()) == OK
    s = host(scratch)
    assert np.isnan(s[need:]).all() and np.isfinite(s[:need]).all()


def both_paths(lib, updates, nc, block):
    """the device SELDMetrics wrapper and direct seld_metrics_update calls, each from a zeroed state: they agree bit for bit"""
    from seld_amd import metrics
    dm = metrics.SELDMetrics(doa_threshold=A.DOA_THRESHOLD, block_size=block, n_classes=nc)
    state = torch.zeros(lib.seld_metrics_state_size(nc), dtype=torch.float64, device="cuda")
    assert dm.state.shape == state.shape and float(dm.state.abs().sum()) == 0.0
    for upd in updates:
        t = [np.array(a) for a in upd]
        dm.update_states(t[:2], t[2:])
        direct_update(lib, state, upd, nc, block)
    got = host(state)
    A.report_exact("wrapper == direct call", host(dm.state), got)
    return dm, got


def check_state(name, got, ref, de_bar):
    """every counter equals the oracle exactly (sums of products of zeros and ones); total_DE within de_bar"""
    assert np.isfinite(got).all()
    keep = np.arange(ref.size) != A.IDX_TOTAL_DE
    A.report_exact(f"{name} counters", got[keep], ref[keep])
    A.report(f"{name} total_DE", abs(got[A.IDX_TOTAL_DE] - ref[A.IDX_TOTAL_DE]), de_bar)


def check_results(name, dm, ref_result, ref_class, de_bar, de_tp):
    """result() and class_result(), compared only after the state: 1e-6 relative on ER, F, DE_F and the class scores, de_bar / DE_TP on DE"""
    ER, F, DE, DE_F = dm.result()
    rER, rF, rDE, rDE_F = ref_result
    for label, g, r in (("ER", ER, rER), ("F", F, rF), ("DE_F", DE_F, rDE_F)):
        A.report(f"{name} {label}", abs(g - r), 1e-6 * abs(r))
    A.report(f"{name} DE", abs(DE - rDE), de_bar / de_tp if de_tp else 0.0)
    for label, g, r in zip(("class recall", "class precision"), dm.class_result(), ref_class):
        assert np.isfinite(g).all()
        with np.errstate(divide="ignore", invalid="ignore"):         # per class; a score of 0 must be 0
            rel = np.where(r != 0, np.abs(g - r) / np.abs(r), np.where(g == 0, 0.0, np.inf))
        A.report(f"{name} {label} (relative)", rel.max(), 1e-6)


@pytest.mark.parametrize("case", A.METRICS_CASES, ids=A.metrics_id)
def test_metrics_update(seld_lib, case):
    name = A.metrics_id(case)
    ref, ref_result, ref_class = A.metrics_reference(case)
    m = A.metrics_margins(case)
    dm, got = both_paths(seld_lib, [A.metrics_inputs(case)], case.nc, case.block)
    check_state(name, got, ref, m.de_bar)
    check_results(name, dm, ref_result, ref_class, m.de_bar, m.de_tp)


def test_metrics_two_updates_accumulate(seld_lib):
    """two updates of different geometry on one state equal the oracle after the same two; reset_states zeroes the state"""
    a, b = A.METRICS_CASES[1], A.MetricsCase(30, 95, 12, 10, 0.25, 40)
    assert a.nc == b.nc and a.block == b.block and b in A.METRICS_CASES
    updates = [A.metrics_inputs(a), A.metrics_inputs(b)]
    om = A.oracle_metrics(updates, a.nc, a.block)
    m = A.margins(updates, a.nc, a.block)
    dm, got = both_paths(seld_lib, updates, a.nc, a.block)
    check_state("two updates", got, om.state_vector(), m.de_bar)
    one, _, _ = A.metrics_reference(a)
    assert got[A.IDX_DE_TP] > one[A.IDX_DE_TP]
    dm.reset_states()
    assert np.array_equal(host(dm.state), np.zeros(got.size))


def test_metrics_hand_built(seld_lib):
    """hand-built tensors at (2, 20, 4, 10): sed_pred exactly 0.5 is not detected and nextafter(0.5, 1) is; a class detected only where it is not
    active adds the extra false negative; an empty block; two directions whose component sums are exactly zero count as distance 0; 19 and 21
    degrees fall on the two sides of doa_threshold = 20.  Counters are held to the hand-worked values as well as to the oracle."""
    c = A.HAND
    upd = [A.hand_built_inputs()]
    om = A.oracle_metrics(upd, c.nc, c.block)
    m = A.margins(upd, c.nc, c.block)
    dm, got = both_paths(seld_lib, upd, c.nc, c.block)
    check_state("hand-built", got, om.state_vector(), m.de_bar)
    for i, k in enumerate(A.STATE_KEYS):
        if k != "total_DE":
            assert got[i] == A.HAND_EXPECTED[k], k
    assert np.array_equal(got[A.MET_SCALARS:], np.concatenate([A.HAND_EXPECTED[k] for k in A.CLASS_KEYS]))
    tp, fp, fn = om.class_tp, om.class_fp, om.class_fn
    check_results("hand-built", dm, om.result(), (A.MO.safe_div(tp, tp + fn), A.MO.safe_div(tp, tp + fp)), m.de_bar, m.de_tp)


def test_metrics_views_of_unsplit_labels(seld_lib):
    """views y[..., :nc], y[..., nc:] of one unsplit [B, S, 4 nc] tensor (the training loop's labels) give the state of contiguous copies"""
    from seld_amd import metrics
    case = A.METRICS_CASES[1]
    sed_t, doa_t, sed_p, doa_p = A.metrics_inputs(case)
    y, yp = dev(np.concatenate([sed_t, doa_t], -1)), dev(np.concatenate([sed_p, doa_p], -1))
    nc = case.nc
    assert not y[..., :nc].is_contiguous() and not y[..., nc:].is_contiguous()
    dm = metrics.SELDMetrics(doa_threshold=A.DOA_THRESHOLD, block_size=case.block, n_classes=nc)
    dm.update_states((y[..., :nc], y[..., nc:]), (yp[..., :nc], yp[..., nc:]))
    _, got = both_paths(seld_lib, [A.metrics_inputs(case)], nc, case.block)
    A.report_exact("views == contiguous copies", host(dm.state), got)
    ref, _, _ = A.metrics_reference(case)
    check_state("views", host(dm.state), ref, A.metrics_margins(case).de_bar)


def test_metrics_empty_state(seld_lib):
    """nothing in the reference and nothing detected: DE = 180 from result(), every block a true negative, no NaN anywhere"""
    B, S, nc, block = 3, 25, 12, 10
    rng = np.random.default_rng(11)
    upd = (np.zeros((B, S, nc), np.float32), np.zeros((B, S, 3 * nc), np.float32),
           (-rng.random((B, S, nc)) - 0.1).astype(np.float32), rng.standard_normal((B, S, 3 * nc)).astype(np.float32))
    om = A.oracle_metrics([upd], nc, block)
    dm, got = both_paths(seld_lib, [upd], nc, block)
    check_state("empty", got, om.state_vector(), 0.0)
    assert got[2] == B * 3 * nc and got.sum() == 2 * B * 3 * nc
    res = dm.result()
    assert res[2] == 180.0 and np.isfinite(res).all() and res == tuple(float(v) for v in om.result())
    assert all(np.isfinite(v).all() for v in dm.class_result())


def test_metrics_bad_class_count(seld_lib):
    """a class count that does not match n_classes raises ValueError and leaves the state untouched"""
    from seld_amd import metrics
    case = A.METRICS_CASES[1]
    upd = [np.array(a) for a in A.metrics_inputs(case)]
    dm = metrics.SELDMetrics(doa_threshold=A.DOA_THRESHOLD, block_size=case.block, n_classes=case.nc)
    dm.update_states(upd[:2], upd[2:])
    before = host(dm.state).copy()
    assert before[7] > 0
    with pytest.raises(ValueError):
        dm.update_states((upd[0][..., :11], upd[1][..., :33]), (upd[2][..., :11], upd[3][..., :33]))
    with pytest.raises(ValueError):
        dm.update_states(upd[:2], (upd[2], upd[3][..., :33]))
    A.report_exact("state after refused updates", host(dm.state), before)


# ---------------------------------------------------------------- frame windows
@pytest.mark.parametrize("kind", ["index", "random"])
@pytest.mark.parametrize("shape", A.FRAME_CASES, ids=str)
def test_frame_windows(seld_lib, shape, kind):
    """bit-exact against infer_oracle.frame; the NaN guard row after the last window stays NaN"""
    T, FC, win, step, first, n = shape
    x = A.frame_inputs(T, FC, kind)
    out = nans(n * win + 1, FC)
    assert seld_lib.seld_frame_windows(ptr(dev(x)), ptr(out), T, FC, win, step, first, n, stream()) == OK
    want = np.concatenate([IO.frame(x, win, step)[first:first + n].reshape(n * win, FC), np.full((1, FC), NAN, np.float32)])
    A.report_exact(f"frame {kind} {shape}", host(out), want)


# ---------------------------------------------------------------- overlap average
def run_overlap(lib, y):
    """the input carries a trailing NaN window and the output a trailing NaN row: neither may be touched"""
    n_win, L, D = y.shape
    yd = torch.cat([dev(y), nans(1, L, D)])
    out = nans(n_win - 1 + L + 1, D)
    assert lib.seld_overlap_average(ptr(yd), ptr(out), n_win, L, D, stream()) == OK
    got = host(out)
    assert np.isnan(got[-1]).all(), "guard row written"
    return got[:-1]


@pytest.mark.parametrize("shape", A.OVERLAP_CASES, ids=str)
def test_overlap_average(seld_lib, shape):
    n_win, L, D = shape
    y = A.overlap_inputs(*shape)
    got = run_overlap(seld_lib, y)
    assert np.isfinite(got).all()
    A.report(f"overlap average {shape}", np.abs(got - IO.overlap_average(y.astype(np.float64))).max(), A.overlap_bar(n_win, L, y))
    # y[w, i, 0] = w: means of consecutive integers are exact, and a sum that starts or stops one window off is not
    yi, want = A.overlap_window_index_inputs(n_win, L)
    A.report_exact(f"overlap window index {shape}", run_overlap(seld_lib, yi), want)


# ---------------------------------------------------------------- augmentation
@pytest.mark.parametrize("mode", A.MASK_MODES)
@pytest.mark.parametrize("shape", A.MASK_CASES, ids=str)
def test_aug_mask(seld_lib, shape, mode):
    """seld_aug_mask with time draws only, frequency draws only and both in one call; then with both pairs null, which leaves x bit-identical"""
    B, T, F, Cc, period = shape
    x, sets = A.mask_inputs(*shape)
    for k, (t_off, t_size, f_off, f_size) in enumerate(sets):
        t = (t_off, t_size) if mode != "freq" else (None, None)
        f = (f_off, f_size) if mode != "time" else (None, None)
        tabs = [idev(a) if a is not None else None for a in (*t, *f)]
        xd = torch.cat([dev(x).reshape(-1), nans(Cc)])
        assert seld_lib.seld_aug_mask(ptr(xd), B, T, F, Cc, period, *(ptr(a) for a in tabs), stream()) == OK
        want = np.concatenate([A.mask_reference(x, period, *t, *f).reshape(-1), np.full(Cc, NAN, np.float32)])
        A.report_exact(f"mask {mode} {shape} draws {k}", host(xd), want)
    xd = dev(x)
    assert seld_lib.seld_aug_mask(ptr(xd), B, T, F, Cc, period, None, None, None, None, stream()) == OK
    A.report_exact(f"mask none {shape}", host(xd), x)


@pytest.mark.parametrize("draw", A.GATHER_DRAWS)
@pytest.mark.parametrize("shape", A.GATHER_CASES, ids=str)
def test_aug_gather_sign(seld_lib, shape, draw):
    B, outer, R, inner = shape
    x, src, sgn = A.gather_inputs(*shape, draw)
    xd = torch.cat([dev(x).reshape(-1), nans(inner)])
    assert seld_lib.seld_aug_gather_sign(ptr(xd), B, outer, R, inner, ptr(idev(src)), ptr(dev(sgn)), stream()) == OK
    want = np.concatenate([A.gather_sign_reference(x, src, sgn).reshape(-1), np.full(inner, NAN, np.float32)])
    A.report_exact(f"gather_sign {draw} {shape}", host(xd), want)


def test_aug_gather_sign_refuses_33_rows(seld_lib):
    """R = 33 is past the register array: SELD_ERR_UNSUPPORTED, and x is left bit-identical"""
    rng = np.random.default_rng(33)
    x = rng.standard_normal((2, 3, 33, 5)).astype(np.float32)
    src, sgn = np.tile(np.arange(33)[::-1], (2, 1)), -np.ones((2, 33), np.float32)
    xd = dev(x)
    assert seld_lib.seld_aug_gather_sign(ptr(xd), 2, 3, 33, 5, ptr(idev(src)), ptr(dev(sgn)), stream()) == UNSUPPORTED
    A.report_exact("gather_sign R=33 leaves x", host(xd), x)


# ---------------------------------------------------------------- feature statistics
def accumulate(lib, acc, scratch, x):
    rows, FC = x.shape
    assert lib.seld_feat_stats_accumulate(ptr(dev(x)), rows, FC, ptr(acc), ptr(scratch), stream()) == OK


def statistics(lib, parts):
    """fold the [rows, FC] tensors into a zeroed accumulator (scratch preset to NaN, of the advertised size plus a guard) -> mean, std, acc"""
    FC = parts[0].shape[1]
    need = lib.seld_feat_stats_scratch_doubles(FC)
    scratch = nans(need + 8, dtype=torch.float64)
    acc = torch.zeros(2 * FC + 1 + 8, dtype=torch.float64, device="cuda")
    acc[2 * FC + 1:] = NAN
    for x in parts:
        accumulate(lib, acc, scratch, x)
    mean, std = nans(FC + 1), nans(FC + 1)
    assert lib.seld_feat_stats_finalize(ptr(acc), FC, ptr(mean), ptr(std), stream()) == OK
    mean, std, a = host(mean), host(std), host(acc)
    assert np.isnan(host(scratch)[need:]).all() and np.isnan(a[2 * FC + 1:]).all() and np.isnan(mean[FC]) and np.isnan(std[FC])
    assert a[2 * FC] == sum(p.shape[0] for p in parts)
    return mean[:FC], std[:FC], a[:2 * FC + 1]


def check_statistics(name, mean, std, x):
    (em, bm), (es, bs) = A.stats_errors(mean, std, A.stats_reference(x))
    A.report(f"{name} mean |got - ref|", em, bm)
    A.report(f"{name} std |got / ref - 1|", es, bs)


@pytest.mark.parametrize("shape", A.STATS_CASES, ids=str)
def test_feat_stats(seld_lib, shape):
    """per column against numpy's fp64 mean / std of the same float32 rows: columns of std 1e-3 .. 1e2 in one tensor, each held to its own bar"""
    x = A.stats_inputs(*shape)
    mean, std, _ = statistics(seld_lib, [x])
    check_statistics(f"stats {shape}", mean, std, x)


def test_feat_stats_two_calls(seld_lib):
    """(8200, 257) + (17, 257) equal numpy on the concatenation, and the same two calls give the same bits on a second run"""
    parts = [A.stats_inputs(8200, 257), A.stats_inputs(*A.STATS_SECOND, seed=1)]
    mean, std, acc = statistics(seld_lib, parts)
    check_statistics("stats two calls", mean, std, np.concatenate(parts))
    mean2, std2, acc2 = statistics(seld_lib, parts)
    A.report_exact("stats second run: accumulator", acc2, acc)
    A.report_exact("stats second run: mean", mean2, mean)
    A.report_exact("stats second run: std", std2, std)


def test_feat_stats_finalize_untouched_accumulator(seld_lib):
    """finalize on a zero accumulator (no rows yet) returns zeros, not 0 / 0"""
    FC = 257
    acc = torch.zeros(2 * FC + 1, dtype=torch.float64, device="cuda")
    mean, std = nans(FC), nans(FC)
    assert seld_lib.seld_feat_stats_finalize(ptr(acc), FC, ptr(mean), ptr(std), stream()) == OK
    A.report_exact("finalize empty: mean", host(mean), np.zeros(FC, np.float32))
    A.report_exact("finalize empty: std", host(std), np.zeros(FC, np.float32))
