"""Cases, seeded inputs and plain numpy references for the small kernels around the train step: metrics.hip (seld_metrics_update), infer.hip
(seld_frame_windows, seld_overlap_average), augment.hip (seld_aug_mask, seld_aug_gather_sign) and feat_stats.hip (seld_feat_stats_*).  Shared by
tests/test_aux_kernels_cpu.py (conditions on the cases, refusals) and tests/test_aux_kernels_gpu.py (the kernels themselves).  Checker only.

Every float input is rounded to float32 before anything is computed from it, so the library and the fp64 references see the same numbers (this
decides `sed_pred > 0.5`).  Inputs and references are cached and returned read-only: compute once, share, leave unchanged."""
import functools
import math
from collections import namedtuple

import numpy as np

from oracle import metrics_oracle as MO
from oracle import seldnet_oracle as O

DOA_THRESHOLD = 20.0
MET_SCALARS = 11          # TP FP TN FN S D I Nref Nsys total_DE DE_TP, then 4 x nc class counters
IDX_TOTAL_DE, IDX_DE_TP = 9, 10
STATE_KEYS = ("TP", "FP", "TN", "FN", "S", "D", "I", "Nref", "Nsys", "total_DE", "DE_TP")
CLASS_KEYS = ("class_tp", "class_fp", "class_tn", "class_fn")


# ---------------------------------------------------------------- reporting, in the style of helpers.check
def report(name, err, bar):
    """one [parity] line: the measured error beside its bar, then the assertion"""
    err, bar = float(err), float(bar)
    ratio = err / bar if bar > 0 else (0.0 if err == 0 else math.inf)
    print(f"[parity] {name:52s} err={err:.3e}  bar={bar:.3e}  err/bar={ratio:.3f}")
    assert np.isfinite(err), f"{name}: non-finite error"
    assert err <= bar, f"{name}: {err:.3e} > bar {bar:.3e}"
    return ratio


def report_exact(name, got, ref):
    """bit-for-bit comparison (NaN equals NaN, as a guard row must stay NaN): prints the number of differing elements"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, f"{name}: shape {got.shape} != {ref.shape}"
    if got.dtype.kind == "f":
        bad = ~((got == ref) | (np.isnan(got) & np.isnan(ref)))
    else:
        bad = got != ref
    n = int(bad.sum())
    print(f"[parity] {name:52s} mismatches={n} of {got.size}  bar=0")
    assert n == 0, f"{name}: {n} of {got.size} elements differ, first at {tuple(np.argwhere(bad)[0]) if got.ndim else ()}"


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


# ---------------------------------------------------------------- metrics: cases and inputs
MetricsCase = namedtuple("MetricsCase", "B S nc block noise seed")
# seeds were picked on the CPU until the conditions of tests/test_aux_kernels_cpu.py::test_metrics_case_conditions held
METRICS_CASES = (
    MetricsCase(1, 1, 1, 1, 0.25, 40),          # smallest possible call
    MetricsCase(3, 25, 12, 10, 0.25, 40),       # ragged last block
    MetricsCase(5, 7, 3, 4, 0.25, 40),          # nc below a quad
    MetricsCase(2, 33, 13, 1, 0.25, 40),        # one frame per block, odd nc
    MetricsCase(2, 64, 14, 32, 0.25, 40),       # largest block
    MetricsCase(30, 95, 12, 10, 0.25, 40),      # 300 items: third block of the items kernel, second stride of the reduce
    MetricsCase(30, 95, 12, 10, 1e-3, 40),      # near-perfect directions: the ill-conditioned end of acosf
    MetricsCase(256, 60, 12, 10, 0.25, 41),     # the training loop's geometry
)


def metrics_id(c):
    return f"B{c.B}-S{c.S}-nc{c.nc}-blk{c.block}-noise{c.noise:g}"


def n_blocks(S, block):
    return (S + block - 1) // block


def state_size(nc):
    return MET_SCALARS + 4 * nc


def tile_classes(sed, doa, nc):
    """labels of 12 classes -> nc classes: the class axis tiled and cut, the same on each of the three DOA component groups [x | y | z]"""
    B, S, n0 = sed.shape
    rep = -(-nc // n0)
    sed_n = np.tile(sed, (1, 1, rep))[..., :nc]
    doa_n = np.tile(doa.reshape(B, S, 3, n0), (1, 1, 1, rep))[..., :nc].reshape(B, S, 3 * nc)
    return np.ascontiguousarray(sed_n), np.ascontiguousarray(doa_n)


@functools.lru_cache(maxsize=None)
def metrics_inputs(case):
    """-> sed_true [B,S,nc], doa_true [B,S,3nc], sed_pred, doa_pred, all float32"""
    _, sed, doa = O.synthetic_batch(case.B, case.S * 5, F_=1, C=1, n_classes=12, seed=case.seed)
    if case.nc != 12:
        sed, doa = tile_classes(sed, doa, case.nc)
    rng = np.random.default_rng([case.seed, 1])
    sed_p = np.clip(0.7 * sed + 0.45 * rng.random(sed.shape), 0, 1).astype(np.float32)
    doa_p = (doa + case.noise * rng.standard_normal(doa.shape)).astype(np.float32)
    return _frozen(sed.astype(np.float32), doa.astype(np.float32), sed_p, doa_p)


def oracle_metrics(updates, nc, block, doa_threshold=DOA_THRESHOLD):
    """oracle.metrics_oracle.SELDMetrics after the given updates [(sed_t, doa_t, sed_p, doa_p), ...]"""
    om = MO.SELDMetrics(doa_threshold=doa_threshold, block_size=block, n_classes=nc)
    for sed_t, doa_t, sed_p, doa_p in updates:
        om.update_states((sed_t, doa_t), (sed_p, doa_p))
    return om


@functools.lru_cache(maxsize=None)
def metrics_reference(case):
    """-> (state vector of the fp64 oracle, result(), (class recall, class precision)) for one update from a zero state"""
    om = oracle_metrics([metrics_inputs(case)], case.nc, case.block)
    tp, fp, fn = om.class_tp, om.class_fp, om.class_fn
    return _frozen(om.state_vector()), tuple(float(v) for v in om.result()), (MO.safe_div(tp, tp + fn), MO.safe_div(tp, tp + fp))


# ---------------------------------------------------------------- metrics: update_block_states restated in a chosen precision
def _l2_normalize(x, eps=1e-12):
    return x / np.sqrt(np.maximum((x ** 2).sum(-1, keepdims=True), eps))


def _distance(xyz0, xyz1, dt):
    xyz0, xyz1 = _l2_normalize(xyz0), _l2_normalize(xyz1)
    zeros = (xyz0.sum(-1) == 0).astype(dt) * (xyz1.sum(-1) == 0).astype(dt)
    d = np.clip((xyz0 * xyz1).sum(-1), -1, 1)
    return np.arccos(d) / np.pi * 180 * (1 - zeros)


def _safe_div(x, y, eps=1e-8):
    return x / np.maximum(y, eps)


def new_state(nc):
    st = {k: 0.0 for k in STATE_KEYS}
    st.update({k: np.zeros(nc) for k in CLASS_KEYS})
    return st


def state_vector(st):
    return np.concatenate([[st[k] for k in STATE_KEYS]] + [st[k] for k in CLASS_KEYS])


def update_block_states(st, tb, pb, doa_threshold, dt):
    """metrics_oracle.SELDMetrics.update_block_states, its statements kept, every array of dtype `dt` (arccos included).  Returns the
    intermediate values the margins are computed from: (frames_matched [B,F,nc], angles [B,F,nc], average_distances [B,nc], exist [B,nc])."""
    sed_true, doa_true = (np.asarray(a, dt) for a in tb)
    sed_pred, doa_pred = (np.asarray(a, dt) for a in pb)
    sed_pred = (sed_pred > 0.5).astype(dt)
    doa_true = np.swapaxes(doa_true.reshape(*doa_true.shape[:-1], 3, -1), -1, -2)
    doa_pred = np.swapaxes(doa_pred.reshape(*doa_pred.shape[:-1], 3, -1), -1, -2)
    true_classes = sed_true.max(-2, keepdims=True)
    pred_classes = sed_pred.max(-2, keepdims=True)
    st["Nref"] += true_classes.sum()
    st["Nsys"] += pred_classes.sum()
    st["TN"] += ((1 - true_classes) * (1 - pred_classes)).sum()
    false_negative = true_classes * (1 - pred_classes)
    false_positive = (1 - true_classes) * pred_classes
    true_negative = (1 - true_classes) * (1 - pred_classes)
    true_positives = true_classes * pred_classes
    st["class_fn"] = st["class_fn"] + false_negative.sum((-3, -2))
    st["class_fp"] = st["class_fp"] + false_positive.sum((-3, -2))
    st["class_tn"] = st["class_tn"] + true_negative.sum((-3, -2))
    st["class_tp"] = st["class_tp"] + true_positives.sum((-3, -2))
    st["FN"] += false_negative.sum()
    st["FP"] += false_positive.sum()
    loc_FN = false_negative.sum((-2, -1))
    loc_FP = false_positive.sum((-2, -1))
    frames_matched = (sed_true * true_positives) * (sed_pred * true_positives)
    total_matched_frames = frames_matched.sum(-2, keepdims=True)
    matched_frames_exist = (total_matched_frames > 0).astype(dt)
    st["DE_TP"] += matched_frames_exist.sum()
    false_negative = true_positives * (1 - matched_frames_exist)
    st["FN"] += false_negative.sum()
    loc_FN = loc_FN + false_negative.sum((-2, -1))
    ang = _distance(doa_true * frames_matched[..., None], doa_pred * frames_matched[..., None], dt)
    average_distances = _safe_div(ang.sum(-2, keepdims=True), total_matched_frames)
    assert ang.dtype == dt and average_distances.dtype == dt
    st["total_DE"] += average_distances.sum()
    close_angles = (average_distances <= doa_threshold).astype(dt)
    st["TP"] += (close_angles * matched_frames_exist).sum()
    false_negative = (1 - close_angles) * matched_frames_exist
    st["FN"] += false_negative.sum()
    loc_FN = loc_FN + false_negative.sum((-2, -1))
    st["S"] += np.minimum(loc_FP, loc_FN).sum()
    st["D"] += np.maximum(0, loc_FN - loc_FP).sum()
    st["I"] += np.maximum(0, loc_FP - loc_FN).sum()
    return frames_matched, ang, average_distances[..., 0, :], matched_frames_exist[..., 0, :]


def restated_metrics(updates, nc, block, dt, doa_threshold=DOA_THRESHOLD):
    """update_states over blocks of `block` frames in precision `dt` -> (state vector, per-block intermediates)"""
    st, probes = new_state(nc), []
    for sed_t, doa_t, sed_p, doa_p in updates:
        for i in range(n_blocks(sed_t.shape[-2], block)):
            sl = slice(i * block, (i + 1) * block)
            probes.append(update_block_states(st, (sed_t[..., sl, :], doa_t[..., sl, :]), (sed_p[..., sl, :], doa_p[..., sl, :]), doa_threshold, dt))
    return np.asarray(state_vector(st), np.float64), probes


Margins = namedtuple("Margins", "threshold sed de_bar de_tp n_close n_far n_half")
DELTA = 4 * 2.0 ** -24      # an fp32 dot product of two fp32-normalised 3-vectors is within this of the exact cosine


def angle_allowance(theta_deg):
    """e(theta): how far an fp32 evaluation of the angle may be from theta [degrees] when its cosine is off by DELTA"""
    th = np.deg2rad(theta_deg)
    return np.rad2deg(np.arccos(np.maximum(np.cos(th) - DELTA, -1.0)) - th)


def margins(updates, nc, block, doa_threshold=DOA_THRESHOLD):
    """From the fp64 restatement's intermediate values (never from the library's output):
      threshold  smallest |average_distance - doa_threshold| over (clip, block, class) items with matched frames
      sed        smallest non-zero |sed_pred - 0.5|; n_half counts the elements exactly at 0.5
      de_bar     2 * sum_items mean_over_matched_frames e(theta) + 1e-5 * DE_TP, the allowance for total_DE
      n_close / n_far   items on either side of the threshold"""
    _, probes = restated_metrics(updates, nc, block, np.float64, doa_threshold)
    thr, allow, de_tp, n_close, n_far = math.inf, 0.0, 0, 0, 0
    for fm, ang, avg, exist in probes:
        on = exist > 0
        if on.any():
            thr = min(thr, float(np.abs(avg[on] - doa_threshold).min()))
        e_item = (angle_allowance(ang) * fm).sum(-2) / np.maximum(fm.sum(-2), 1.0)
        allow += float(e_item[on].sum())
        de_tp += int(on.sum())
        n_close += int((on & (avg <= doa_threshold)).sum())
        n_far += int((on & (avg > doa_threshold)).sum())
    d = np.concatenate([np.abs(np.asarray(u[2], np.float64) - 0.5).ravel() for u in updates])
    return Margins(thr, float(d[d > 0].min()), 2 * allow + 1e-5 * de_tp, de_tp, n_close, n_far, int((d == 0).sum()))


@functools.lru_cache(maxsize=None)
def metrics_margins(case):
    return margins([metrics_inputs(case)], case.nc, case.block)


# ---------------------------------------------------------------- metrics: hand-built tensors at (2, 20, 4, 10)
HAND = MetricsCase(2, 20, 4, 10, None, 7)
# worked by hand from metrics_oracle.update_block_states; tests/test_aux_kernels_cpu.py holds the oracle to it
HAND_EXPECTED = dict(TP=3, FP=1, TN=8, FN=4, S=1, D=3, I=0, Nref=7, Nsys=6, DE_TP=4,
                     class_tp=[2, 2, 0, 1], class_fp=[0, 0, 1, 0], class_tn=[2, 2, 2, 2], class_fn=[0, 0, 1, 1])


@functools.lru_cache(maxsize=None)
def hand_built_inputs():
    """item (clip 0, block 0): class 0 predicted 19 deg off its reference, class 1 21 deg off (the two sides of doa_threshold = 20), class 2 predicted
    at exactly 0.5 (not detected), class 3 at nextafter(0.5, 1) (detected).  (0, 1): class 0 active in frames 10-12 and detected only in 15-17
    (no matched frame: the extra false negative), class 1 with doa_true (1,-1,0)/sqrt2 against doa_pred (0,1,-1)/sqrt2 (both component sums
    exactly zero: the reference counts the distance as 0, not 120 deg).  (1, 0): nothing at all.  (1, 1): one false positive, one miss.
    doa_pred is noise wherever nothing is matched: it must be ignored there."""
    B, S, nc, _, _, seed = HAND
    rng = np.random.default_rng(seed)
    sed_t = np.zeros((B, S, nc), np.float32)
    doa_t = np.zeros((B, S, 3, nc), np.float32)
    sed_p = np.full((B, S, nc), 0.1, np.float32)
    doa_p = rng.standard_normal((B, S, 3, nc)).astype(np.float32)
    for c, deg in ((0, 19.0), (1, 21.0)):
        sed_t[0, 0:5, c] = 1
        sed_p[0, 0:5, c] = 0.9
        doa_t[0, 0:5, :, c] = (1, 0, 0)
        doa_p[0, 0:5, :, c] = (math.cos(math.radians(deg)), math.sin(math.radians(deg)), 0)
    sed_t[0, 3, 2] = 1
    sed_p[0, 3, 2] = 0.5
    doa_t[0, 3, :, 2] = (0, 1, 0)
    sed_t[0, 3, 3] = 1
    sed_p[0, 3, 3] = np.nextafter(np.float32(0.5), np.float32(1))
    doa_t[0, 3, :, 3] = doa_p[0, 3, :, 3] = (0, 0, 1)
    sed_t[0, 10:13, 0] = 1
    sed_p[0, 15:18, 0] = 0.8
    doa_t[0, 10:13, :, 0] = (0, 0, -1)
    r = np.float32(1 / math.sqrt(2))
    sed_t[0, 11, 1] = 1
    sed_p[0, 11, 1] = 0.7
    doa_t[0, 11, :, 1] = (r, -r, 0)
    doa_p[0, 11, :, 1] = (0, r, -r)
    sed_p[1, 15, 2] = 0.6
    sed_t[1, 12, 3] = 1
    doa_t[1, 12, :, 3] = (0, 1, 0)
    assert sed_p[0, 3, 2] == 0.5 and sed_p[0, 3, 3] > 0.5
    return _frozen(sed_t, doa_t.reshape(B, S, 3 * nc), sed_p, doa_p.reshape(B, S, 3 * nc))


# ---------------------------------------------------------------- frame windows
# (T, FC, win, step, first, n)
FRAME_CASES = (
    (23, 4, 5, 3, 0, 7),            # last window ends at 22
    (23, 4, 5, 3, 2, 5),            # a later batch of the same clip
    (50, 448, 10, 5, 0, 9),
    (37, 12, 37, 1, 0, 1),          # the window is the clip
    (300, 64, 7, 7, 1, 41),         # no overlap; total4 is not a multiple of 256
)


@functools.lru_cache(maxsize=None)
def frame_inputs(T, FC, kind):
    """kind 'index': x[t, j] = t*FC + j (exact in float32); 'random': N(0,1)"""
    if kind == "index":
        x = np.arange(T * FC, dtype=np.float32).reshape(T, FC)
        assert T * FC < 2 ** 24
    else:
        x = np.random.default_rng([T, FC]).standard_normal((T, FC)).astype(np.float32)
    return _frozen(x)


# ---------------------------------------------------------------- overlap average
# (n_win, L, D)
OVERLAP_CASES = (
    (1, 6, 12), (6, 1, 36),
    (7, 9, 5), (8, 9, 5), (9, 9, 5),                # the unroll edge
    (20, 12, 36), (12, 20, 36),                     # counts plateau at L, resp. at n_win
    (19, 17, 3),                                    # two unrolled rounds plus a tail
    (41, 10, 257),                                  # D over one thread block
)


@functools.lru_cache(maxsize=None)
def overlap_inputs(n_win, L, D):
    return _frozen(np.random.default_rng([n_win, L, D]).standard_normal((n_win, L, D)).astype(np.float32))


def overlap_window_index_inputs(n_win, L):
    """y[w, i, 0] = w: every output is a mean of consecutive integers, (lo + hi) / 2, exact in float32"""
    y = np.broadcast_to(np.arange(n_win, dtype=np.float32)[:, None, None], (n_win, L, 1)).copy()
    t = np.arange(n_win - 1 + L)
    lo, hi = np.maximum(0, t - L + 1), np.minimum(n_win - 1, t)
    return y, ((lo + hi) / 2.0).astype(np.float32)[:, None]


def overlap_bar(n_win, L, y):
    """a sequential fp32 sum of min(n_win, L) terms plus one division"""
    return min(n_win, L) * 2.0 ** -24 * float(np.abs(y).max())


# ---------------------------------------------------------------- augmentation
# (B, T, F, C, period)
MASK_CASES = ((2, 20, 8, 7, 10), (3, 12, 5, 10, 4), (1, 6, 3, 17, 6), (4, 300, 64, 7, 100))
MASK_MODES = ("time", "freq", "both")
# (B, outer, R, inner)
GATHER_CASES = ((2, 3, 1, 1), (3, 5, 4, 12), (2, 7, 7, 1), (2, 300, 17, 1), (2, 3, 32, 5), (1, 1, 32, 1))
GATHER_DRAWS = ("permutation", "repeats", "identity")


def _mask_draws(rng, n, total, special):
    """n (offset, size) int32 draws with offset + size <= total; `special` replaces the first draws"""
    size = rng.integers(0, total + 1, n)
    off = (rng.random(n) * (total - size + 1)).astype(np.int64)
    for i, (o, s) in enumerate(special):
        off[i], size[i] = o, s
    assert (off >= 0).all() and (off + size <= total).all()
    return off.astype(np.int32), size.astype(np.int32)


@functools.lru_cache(maxsize=None)
def mask_inputs(B, T, F, C, period):
    """-> x [B,T,F,C] and a list of draw sets (t_off, t_size, f_off, f_size), each [B * T/period].  Over the list, each axis holds a size-0
    draw (at a non-zero offset), a mask that ends exactly at the edge (`period`, resp. F) and a full-length mask; a shape with fewer than
    three segments gets as many draw sets as it takes."""
    rng = np.random.default_rng([B, T, F, C, period])
    x = rng.standard_normal((B, T, F, C)).astype(np.float32)
    x[x == 0] = 1.0                     # a zero in the input would hide a missed mask
    n = B * (T // period)

    def special(total):
        k = max(1, total // 3)
        return [(min(1, total - 1), 0), (total - k, k), (0, total)]

    sets = []
    ts, fs = special(period), special(F)
    fs = fs[1:] + fs[:1]                # rotated: a size-0 draw on one axis never meets a full-length mask on the other, which would hide it
    for j in range(0, 3, n):
        sets.append(_mask_draws(rng, n, period, ts[j:j + n]) + _mask_draws(rng, n, F, fs[j:j + n]))
    return _frozen(x), sets


def mask_reference(x, period, t_off=None, t_size=None, f_off=None, f_size=None):
    """seld_aug_mask as include/seld_hip.h states it, either pair optional: frames [t_off, t_off + t_size) of each period-frame segment and
    bins [f_off, f_off + f_size) of every frame of the segment are zeroed"""
    x = np.array(x, copy=True)
    B, T = x.shape[:2]
    nseg = T // period
    for b in range(B):
        for s in range(nseg):
            seg = x[b, s * period:(s + 1) * period]
            if t_off is not None:
                seg[t_off[b * nseg + s]:t_off[b * nseg + s] + t_size[b * nseg + s]] = 0
            if f_off is not None:
                seg[:, f_off[b * nseg + s]:f_off[b * nseg + s] + f_size[b * nseg + s]] = 0
    return x


@functools.lru_cache(maxsize=None)
def gather_inputs(B, outer, R, inner, draw):
    """-> x [B, outer, R, inner], src int32 [B, R], sgn float32 [B, R] of +-1"""
    rng = np.random.default_rng([B, outer, R, inner, GATHER_DRAWS.index(draw)])
    x = rng.standard_normal((B, outer, R, inner)).astype(np.float32)
    if draw == "permutation":
        src = np.stack([rng.permutation(R) for _ in range(B)])
    elif draw == "repeats":
        src = rng.integers(0, R, (B, R))
    else:
        src = np.tile(np.arange(R), (B, 1))
    sgn = rng.choice(np.array([-1.0, 1.0], np.float32), (B, R))
    return _frozen(x, src.astype(np.int32), sgn.astype(np.float32))


def gather_sign_reference(x, src, sgn):
    """out[b, o, r, i] = sgn[b, r] * x[b, o, src[b, r], i]"""
    b = np.arange(x.shape[0])[:, None]
    return (x.transpose(0, 2, 1, 3)[b, src] * sgn[:, :, None, None]).transpose(0, 2, 1, 3)


# ---------------------------------------------------------------- feature statistics
# (rows, FC)
STATS_CASES = (
    (1, 1),
    (15, 448), (16, 448), (17, 448),                # one and two chunks
    (8192, 4),                                      # exactly the 512-chunk cap
    (8193, 640),
    (8200, 257),                                    # chunks of 17 rows: the last 29 of 512 blocks are empty
    (20000, 1088),                                  # a thread owns several columns
)
STATS_SECOND = (17, 257)                            # a second accumulate call after (8200, 257)


@functools.lru_cache(maxsize=None)
def stats_inputs(rows, FC, seed=0):
    """columns with std from 1e-3 to 1e2 and mean offsets up to 100, all in one tensor; column 0 is the hardest pairing (std 1e-3 at mean 100)"""
    rng = np.random.default_rng([rows, FC, seed])
    std = 10.0 ** rng.uniform(-3, 2, FC)
    mean = rng.uniform(-100, 100, FC)
    std[0], mean[0] = 1e-3, 100.0
    if FC > 1:
        std[-1], mean[-1] = 1e2, 0.0
    return _frozen((mean + std * rng.standard_normal((rows, FC))).astype(np.float32))


def stats_reference(x):
    """numpy mean / std (ddof 0) in fp64 of the float32 rows, per column, with the bars they are held to:
      mean  |got - ref| <= 2^-23 |ref| + n 2^-53 max|x|                 (float rounding of the result + a worst-case double sum of n rows)
      std   |got / ref - 1| <= 2^-22 + n 2^-53 (1 + (mean / std)^2)     (float rounding + the cancellation in E[x^2] - m^2)
    max|x| is taken per column.  A column of zero reference std (one row: s2 / 1 - m * m is exactly 0 in double, the square of a float32 being
    exact there) has std bar 0."""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    m, s = x.mean(0), x.std(0)
    mean_bar = 2.0 ** -23 * np.abs(m) + n * 2.0 ** -53 * np.abs(x).max(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        std_bar = np.where(s > 0, 2.0 ** -22 + n * 2.0 ** -53 * (1 + (m / s) ** 2), 0.0)
    return m, s, mean_bar, std_bar


def _worst_column(err, bar):
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bar > 0, err / bar, np.where(err == 0, 0.0, np.inf))
    assert not np.isnan(ratio).any()
    i = int(np.argmax(ratio))
    return float(err[i]), float(bar[i])


def stats_errors(mean, std, ref):
    """-> ((err, bar) of the mean, (err, bar) of the std), each at the column closest to (or furthest over) its bar; err is the quantity the
    bar is stated on: |got - ref| for the mean, |got / ref - 1| for the std (|got| where the reference std is 0)"""
    m, s, mean_bar, std_bar = ref
    mean, std = np.asarray(mean, np.float64).ravel(), np.asarray(std, np.float64).ravel()
    assert np.isfinite(mean).all() and np.isfinite(std).all()
    with np.errstate(divide="ignore", invalid="ignore"):
        es = np.where(s > 0, np.abs(std / s - 1), np.abs(std))
    return _worst_column(np.abs(mean - m), mean_bar), _worst_column(es, std_bar)
