"""Checker only: a numpy + scipy restatement of the reference's dict-based DCASE scoring path, and the seeded case generator of the
dcase tests.  Nothing here is imported by seld_amd.

  load_csv                    utils.load_output_format_file            utils.py:271-291
  polar_to_cartesian          utils.convert_output_format_polar_to_cartesian   utils.py:352-367
  segment_labels              utils.segment_labels                     utils.py:293-324
  angle                       distance_between_cartesian_coordinates   SELD_evaluation_metrics.py:171-188
  assign                      least_distance_between_gt_pred           SELD_evaluation_metrics.py:191-220 (the Hungarian assignment is kept)
  Scorer.update / .scores     SELDMetrics_.update_seld_scores / compute_seld_scores   SELD_evaluation_metrics.py:63-154, 48-61
  seld_score                  metrics.calculate_seld_score             metrics.py:157-170
"""
import numpy as np
from scipy.optimize import linear_sum_assignment

EPS = np.finfo(float).eps
NAMES = ("TP", "FP", "FN", "S", "D", "I", "Nref", "total_DE", "DE_TP", "DE_FP", "DE_FN")


def load_csv(path):
    out = {}
    with open(path) as fid:
        for line in fid:
            w = line.strip().split(",")
            frame = int(float(w[0]))
            if len(w) == 5:
                out.setdefault(frame, []).append([int(float(w[1])), float(w[3]), float(w[4]), int(float(w[2]))])
            elif len(w) == 6:
                out.setdefault(frame, []).append([int(float(w[1])), float(w[3]), float(w[4]), float(w[5]), int(float(w[2]))])
    return out


def polar_to_cartesian(d):
    out = {}
    for frame, rows in d.items():
        out[frame] = []
        for cls, azi, ele, track in rows:
            e, a = ele * np.pi / 180., azi * np.pi / 180
            c = np.cos(e)
            out[frame].append([cls, np.cos(a) * c, np.sin(a) * c, np.sin(e), track])
    return out


def segment_labels(d, max_frames, seg=10):
    """-> {segment: {class: [[frames-in-segment], [rows-without-class per frame]]}}; the reference wraps the pair in a one-element list,
    which its reader undoes with [0]"""
    out = {b: {} for b in range(int(np.ceil(max_frames / float(seg))))}
    for f0 in range(0, max_frames, seg):
        loc = {}
        for frame in range(f0, f0 + seg):
            for row in d.get(frame, []):
                loc.setdefault(row[0], {}).setdefault(frame - f0, []).append(row[1:])
        for cls, frames in loc.items():
            out[f0 // seg][cls] = [list(frames.keys()), list(frames.values())]
    return out


def angle(x1, y1, z1, x2, y2, z2):
    n1 = np.sqrt(x1 ** 2 + y1 ** 2 + z1 ** 2 + 1e-10)
    n2 = np.sqrt(x2 ** 2 + y2 ** 2 + z2 ** 2 + 1e-10)
    x1, y1, z1, x2, y2, z2 = x1 / n1, y1 / n1, z1 / n1, x2 / n2, y2 / n2, z2 / n2
    dist = np.clip(x1 * x2 + y1 * y2 + z1 * z2, -1, 1)
    return np.arccos(dist) * 180 / np.pi


def assign(gt_xyz, pred_xyz):
    """cost matrix [n_gt, n_pred] of angles, Hungarian assignment -> (costs, gt rows, pred columns)"""
    g, p = np.asarray(gt_xyz, float), np.asarray(pred_xyz, float)
    cost = np.zeros((len(g), len(p)))
    for i in range(len(g)):
        for j in range(len(p)):
            cost[i, j] = angle(g[i, 0], g[i, 1], g[i, 2], p[j, 0], p[j, 1], p[j, 2])
    rows, cols = linear_sum_assignment(cost)
    return cost[rows, cols], rows, cols, cost


class Scorer:
    def __init__(self, doa_threshold=20, nb_classes=11):
        self.T, self.nc = doa_threshold, nb_classes
        self.c = dict.fromkeys(NAMES, 0)
        self.track_avgs = []          # every track average compared with the threshold
        self.tie_gaps = []            # per scored frame with several entries: second smallest - smallest distance

    def update(self, pred, gt):
        """pred, gt: segment_labels outputs of one file, cartesian rows [x, y, z, track]"""
        c = self.c
        for b in range(len(gt)):
            loc_fn = loc_fp = 0
            for k in range(self.nc):
                if k in gt[b]:
                    c["Nref"] += max(len(v) for v in gt[b][k][1])
                if k in gt[b] and k in pred[b]:
                    dist, cnt = {}, {}
                    gframes, pframes = gt[b][k][0], pred[b][k][0]
                    for gi, gf in enumerate(gframes):
                        if gf not in pframes:
                            continue
                        garr = np.array(gt[b][k][1][gi], float)
                        parr = np.array(pred[b][k][1][pframes.index(gf)], float)
                        costs, rows, _, full = assign(garr[:, :-1], parr[:, :-1])
                        if full.shape[0] > 1 and full.shape[1] == 1:
                            s = np.sort(full[:, 0])
                            self.tie_gaps.append(s[1] - s[0])
                        for d, r in zip(costs, rows):
                            tid = garr[r, -1]
                            dist.setdefault(tid, []).append(d)
                            cnt[tid] = cnt.get(tid, 0) + 1
                    if not dist:
                        loc_fn += 1; c["FN"] += 1; c["DE_FN"] += 1
                    else:
                        for tid in dist:
                            avg = sum(dist[tid]) / cnt[tid]
                            self.track_avgs.append(avg)
                            c["total_DE"] += avg
                            c["DE_TP"] += 1
                            if avg <= self.T:
                                c["TP"] += 1
                            else:
                                loc_fp += 1; c["FP"] += 1
                elif k in gt[b]:
                    loc_fn += 1; c["FN"] += 1; c["DE_FN"] += 1
                elif k in pred[b]:
                    loc_fp += 1; c["FP"] += 1; c["DE_FP"] += 1
            c["S"] += min(loc_fp, loc_fn)
            c["D"] += max(0, loc_fn - loc_fp)
            c["I"] += max(0, loc_fp - loc_fn)

    def state(self):
        return np.array([self.c[n] for n in NAMES], float)

    def scores(self):
        return scores_from_state(self.state())


def scores_from_state(state):
    TP, FP, FN, S, D, I, Nref, total_DE, DE_TP, DE_FP, DE_FN = (float(v) for v in state)
    ER = (S + D + I) / float(Nref + EPS)
    F = TP / (EPS + TP + 0.5 * (FP + FN))
    LE = total_DE / float(DE_TP + EPS) if DE_TP else 180
    LR = DE_TP / (EPS + DE_TP + DE_FN)
    return ER, F, LE, LR


def seld_score(m):
    return (m[0] + 1 - m[1] + m[2] / 180 + 1 - m[3]) / 4


def pred_dict(sed, doa, thr=0.5):
    """model-format outputs of one file -> what write_answer followed by load_csv gives: {frame: [[class, x, y, z, 0]]}"""
    sed, doa = np.asarray(sed, np.float32), np.asarray(doa, np.float32)
    nc = sed.shape[1]
    thr = np.broadcast_to(np.asarray(thr, np.float32), (nc,))
    out = {}
    for t, c in zip(*np.nonzero(sed > thr[None])):
        out.setdefault(int(t), []).append([int(c), float(doa[t, c]), float(doa[t, nc + c]), float(doa[t, 2 * nc + c]), 0])
    return out


def score_files(files, thr=0.5, doa_threshold=20, nb_classes=None):
    """files: [(sed, doa, gt cartesian dict)] -> the Scorer after all of them"""
    sc = Scorer(doa_threshold, nb_classes if nb_classes is not None else files[0][0].shape[1])
    for sed, doa, gt in files:
        T = sed.shape[0]
        sc.update(segment_labels(pred_dict(sed, doa, thr), T), segment_labels(gt, T))
    return sc


# ---------------------------------------------------------------- the hand-worked case
def _unit(azi, ele=0):
    a, e = azi * np.pi / 180, ele * np.pi / 180
    return np.array([np.cos(a) * np.cos(e), np.sin(a) * np.cos(e), np.sin(e)])


def hand_case(tail=False):
    """One file, 2 classes, threshold 20 degrees; 20 frames, or 23 with `tail` (a ragged 3-frame last segment).
      segment 0, class 0: both present, tracks 3 (azimuth 0) and 7 (azimuth 90) in frames 0-2; predictions at azimuth 0, 50, 30 in those
                          frames and one more in frame 5, where there is no reference.  Frame 0 -> track 3 at 0, frame 1 -> track 7 at 40,
                          frame 2 -> track 3 at 30: track 3 averages 15 (TP), track 7 averages 40 (FP, loc_FP).  Nref += 2.
      segment 0, class 1: reference only (frame 4): FN, DE_FN, loc_FN.  Nref += 1.               -> S += 1
      segment 1, class 0: prediction only (frame 12): FP, DE_FP, loc_FP.
      segment 1, class 1: reference in frame 10, prediction in frame 15: no common frame: FN, DE_FN, loc_FN.  Nref += 1.   -> S += 1
      tail,      class 0: reference in frames 20 and 21 (two entries in 21: elevation 90 and azimuth 0), prediction in 21 straight up:
                          track 1 at 0 (TP).  Nref += 2.
      tail,      class 1: prediction only (frame 22): FP, DE_FP, loc_FP.                          -> I += 1
    A distance "0" is 8.1e-4 degrees: the 1e-10 under the square root shortens both unit vectors (SELD_evaluation_metrics.py:180-181).
    -> (sed, doa, gt cartesian, gt polar, expected counters)"""
    T, nc = (23 if tail else 20), 2
    sed = np.full((T, nc), 0.1, np.float32)
    doa = np.zeros((T, 3 * nc), np.float32)
    gt = {0: [[0, 0, 0, 3], [0, 90, 0, 7]], 1: [[0, 0, 0, 3], [0, 90, 0, 7]], 2: [[0, 0, 0, 3], [0, 90, 0, 7]], 4: [[1, -120, 30, 0]],
          10: [[1, 10, 10, 2]]}
    for t, c, azi, ele in ((0, 0, 0, 0), (1, 0, 50, 0), (2, 0, 30, 0), (5, 0, 77, 5), (12, 0, -60, 20), (15, 1, 10, 10)):
        sed[t, c] = 0.9
        doa[t, c::nc] = _unit(azi, ele)
    want = dict(TP=1, FP=2, FN=2, S=2, D=0, I=0, Nref=4, total_DE=55.0, DE_TP=2, DE_FP=1, DE_FN=2)
    if tail:
        gt[20] = [[0, 45, 0, 1]]
        gt[21] = [[0, 0, 90, 1], [0, 0, 0, 2]]
        sed[21, 0] = sed[22, 1] = 0.9
        doa[21, 0::nc] = (0, 0, 1)
        doa[22, 1::nc] = _unit(5, 5)
        want = dict(TP=2, FP=3, FN=2, S=2, D=0, I=1, Nref=6, total_DE=55.0, DE_TP=3, DE_FP=2, DE_FN=2)
    return sed, doa, polar_to_cartesian(gt), gt, want


# ---------------------------------------------------------------- the seeded case generator
SIGMAS = (0.05, 0.3, 1.0)
MARGIN_DEG = 1e-3
MAX_REDRAWS = 5


def _draw(files, T, nc, K, seed, thr):
    rng = np.random.default_rng(seed)
    thr = np.broadcast_to(np.asarray(thr, np.float32), (nc,))
    sigma = rng.choice(SIGMAS, nc)
    out = []
    for _ in range(files):
        act = np.zeros((T, nc), bool)
        doa = rng.standard_normal((T, 3 * nc))                    # pure noise wherever no reference entry is followed
        gt = {}
        for t0 in range(0, T, 10):
            n = min(10, T - t0)
            for c in range(nc):
                g_on = rng.random() < 0.5
                p_on = rng.random() < (0.6 if g_on else 0.15)
                g_fr = rng.random(n) < 0.8 if g_on else np.zeros(n, bool)
                p_fr = rng.random(n) < 0.8 if p_on else np.zeros(n, bool)
                act[t0:t0 + n, c] = p_fr
                for f in np.nonzero(g_fr)[0]:
                    k = int(rng.integers(1, K + 1))
                    ids = rng.permutation(min(8, K + 2))[:k]
                    for tid in ids:
                        azi, ele = int(rng.integers(-180, 180)), int(rng.integers(-45, 46))
                        gt.setdefault(t0 + int(f), []).append([c, azi, ele, int(tid)])
                    e, a = ele * np.pi / 180, azi * np.pi / 180      # the prediction follows the frame's last entry
                    unit = np.array([np.cos(a) * np.cos(e), np.sin(a) * np.cos(e), np.sin(e)])
                    if rng.random() < 0.9:
                        doa[t0 + f, c::nc] = unit + sigma[c] * rng.standard_normal(3)
        u = rng.random((T, nc))
        sed = np.where(act, thr + (1 - thr) * (0.1 + 0.9 * u), thr * 0.9 * u)
        out.append((sed.astype(np.float32), doa.astype(np.float32), polar_to_cartesian(gt), gt))
    return out


def make_case(files, T, nc, K, seed=0, thr=0.5, doa_threshold=20):
    """-> (files [(sed, doa, gt cartesian dict, gt polar dict)], Scorer of the oracle).  A draw is rejected, and the next seed taken, when a
    track's average lies within MARGIN_DEG of the threshold or two entries of one (frame, class) are within MARGIN_DEG of being
    equidistant from the prediction: there a correct scorer in another summation order may decide the other way."""
    for redraw in range(MAX_REDRAWS + 1):
        case = _draw(files, T, nc, K, seed + 1000 * redraw, thr)
        sc = score_files([f[:3] for f in case], thr, doa_threshold, nc)
        near_thr = [a for a in sc.track_avgs if abs(a - doa_threshold) < MARGIN_DEG]
        near_tie = [g for g in sc.tie_gaps if g < MARGIN_DEG]
        if not near_thr and not near_tie:
            return case, sc
    raise AssertionError("no draw with decision margins in %d redraws" % MAX_REDRAWS)


def write_metadata_csv(path, gt_polar):
    """a DCASE metadata file: frame, class, track, azimuth, elevation"""
    with open(path, "w") as fid:
        for frame in sorted(gt_polar):
            for cls, azi, ele, track in gt_polar[frame]:
                fid.write(f"{frame},{cls},{track},{azi},{ele}\n")
