"""Checker only: the seeded cases of the threshold-sweep tests (test_dcase_sweep_cpu.py, test_dcase_sweep_gpu.py) and the oracle-driven sweep,
built on tests/dcase_oracle.py.  Nothing here is imported by seld_amd.

A case is (files, T, nc, K) with a candidate list and a named seed.  The reference tracks, the predicted DOAs and which frames are meant to be
active come from DO._draw; `sed` is drawn here, spread across the candidate range around a per-class centre (DO._draw clusters it around the
one threshold it is given, so no candidate but that one would change a decision).

A draw is rejected when a correct scorer in another summation order could decide differently from the oracle anywhere the test looks:
  * a track average of any row within DO.MARGIN_DEG of the DOA threshold, or two entries of a (frame, class) within DO.MARGIN_DEG of being
    equidistant from the prediction;
  * two rows of one sweep whose counters differ and whose scores are within SCORE_MARGIN of each other: choose_step could pick either.
    SCORE_MARGIN = 1e-7: total_DE may differ by 1e-5 degrees per averaged track between two correct scorers (test_dcase_gpu.py), so LE by
    1e-5 degrees and the score by 1e-5 / 180 / 4 = 1.4e-8 per row, 2.8e-8 between two rows.  This covers the 1e-9 between rows with
    different integer counters and also rows that differ in total_DE alone.
Every named seed is accepted at the first draw (test_dcase_sweep_cpu.py asserts it)."""
import functools

import numpy as np

import dcase_oracle as DO

BASE_THRESHOLD = (0.3, 0.35, 0.4, 0.45, 0.55, 0.6, 0.65, 0.7)      # the reference's search_best.py:145
DOA_THRESHOLD = 20
SCORE_MARGIN = 1e-7
MAX_REDRAWS = 5
LINSPACE12 = tuple(np.linspace(0.2, 0.8, 12).astype(np.float32).tolist())

# (files, T, nc, K), candidates, base table -> seed: one sweep at the base table
SWEEP_CASES = {
    "two_files": ((2, 23, 3, 2), (0.35, 0.5, 0.65), 0.5, 1),
    "one_segment": ((1, 7, 1, 4), (0.6,), 0.5, 3),          # seed 3: three averaged tracks at 0.5, one at 0.6
    "twelve_classes": ((3, 53, 12, 3), BASE_THRESHOLD, LINSPACE12, 0),
}
# (files, T, nc, K), candidates, start -> seed: every sweep of the whole search
SEARCH_CASES = {
    "two_files": ((2, 23, 3, 2), (0.35, 0.5, 0.65), 0.5, 1),
    "six_classes": ((3, 53, 6, 2), BASE_THRESHOLD, 0.5, 0),
}


def draw(files, T, nc, K, seed):
    """-> [(sed, doa, gt cartesian, gt polar)]: DO._draw's tracks and DOAs, `sed` redrawn around a per-class centre in 0.35..0.65: frames
    meant active lie 0.1 below to 0.35 above it, the others 0.1 above to 0.35 below, so the two overlap and every candidate moves counts"""
    base = DO._draw(files, T, nc, K, seed, 0.5)
    rng = np.random.default_rng([seed, 77])
    centre = rng.uniform(0.35, 0.65, nc)
    out = []
    for sed, doa, gt, gt_polar in base:
        act = sed > 0.5
        u = rng.uniform(-0.1, 0.35, sed.shape)
        new = np.clip(np.where(act, centre + u, centre - u), 0.01, 0.99).astype(np.float32)
        out.append((new, doa, gt, gt_polar))
    return out


def row_thresholds(base, cand, nc):
    """the nc * M + 1 threshold vectors of one sweep, in table order (the last one is the base)"""
    base = np.broadcast_to(np.asarray(base, np.float32), (nc,)).copy()
    rows = []
    for c in range(nc):
        for v in cand:
            t = base.copy()
            t[c] = np.float32(v)
            rows.append(t)
    rows.append(base)
    return rows


class OracleSweep:
    """thr -> (table [nc, M, 11], base [11]) from DO.score_files, one call per row; keeps every row's Scorer for the margin checks"""

    def __init__(self, files, nc, cand, doa_threshold=DOA_THRESHOLD):
        self.files, self.nc, self.cand, self.T = [f[:3] for f in files], nc, tuple(cand), doa_threshold
        self.sweeps = []          # per call: [(thr, Scorer)] in table order
        self._memo = {}

    def _score(self, thr):
        key = thr.tobytes()
        if key not in self._memo:
            self._memo[key] = DO.score_files(self.files, thr, self.T, self.nc)
        return self._memo[key]

    def __call__(self, thr):
        rows = [(t, self._score(t)) for t in row_thresholds(thr, self.cand, self.nc)]
        self.sweeps.append(rows)
        states = np.array([sc.state() for _, sc in rows])
        return states[:-1].reshape(self.nc, len(self.cand), 11), states[-1]


def objection(sweeps, doa_threshold=DOA_THRESHOLD, choice=True):
    """why a draw is rejected, or None; with choice=False only the rows' counters are asked about, not the choice between rows"""
    for rows in sweeps:
        for _, sc in rows:
            if any(abs(a - doa_threshold) < DO.MARGIN_DEG for a in sc.track_avgs):
                return "a track average at the DOA threshold"
            if any(g < DO.MARGIN_DEG for g in sc.tie_gaps):
                return "a near-equidistant pair"
        if not choice:
            continue
        states = [sc.state() for _, sc in rows]
        scores = [DO.seld_score(DO.scores_from_state(s)) for s in states]
        order = np.argsort(scores)
        for a, b in zip(order[:-1], order[1:]):          # identical rows may sit between two near ones: compare each with its next different
            if scores[b] - scores[a] < SCORE_MARGIN and not np.array_equal(states[a], states[b]):
                return "two different rows with near-equal scores"
    return None


def _accepted(shape, seed, run):
    for redraw in range(MAX_REDRAWS + 1):
        files = draw(*shape, seed=seed + 1000 * redraw)
        got = run(files)
        why = objection(got[0].sweeps)
        if why is None:
            return (files, redraw) + got
    raise AssertionError("no draw with decision margins in %d redraws (%s)" % (MAX_REDRAWS, why))


@functools.lru_cache(maxsize=None)
def sweep_case(name):
    """-> (files, redraws, OracleSweep after one call, table, base) of SWEEP_CASES[name]"""
    shape, cand, base, seed = SWEEP_CASES[name]

    def run(files):
        o = OracleSweep(files, shape[2], cand)
        table, b = o(np.broadcast_to(np.asarray(base, np.float32), (shape[2],)).copy())
        return o, table, b
    return _accepted(shape, seed, run)


@functools.lru_cache(maxsize=None)
def search_case(name):
    """-> (files, redraws, OracleSweep after the search, (thresholds, score, metrics, steps)) of SEARCH_CASES[name]: search_thresholds
    driven by the oracle"""
    from seld_amd import search_best
    shape, cand, start, seed = SEARCH_CASES[name]

    def run(files):
        o = OracleSweep(files, shape[2], cand)
        return o, search_best.search_thresholds(None, None, cand, start, DOA_THRESHOLD, shape[2], sweep=o)
    return _accepted(shape, seed, run)
