"""The hand-built cases of tests/test_tdm_gpu.py, kept apart so that tests/test_tdm_cpu.py can check, without a GPU, that each plan meets the
situation it is there for (through tests/tdm_oracle.py).  Everything is generated from fixed seeds; nothing here touches the device."""
import numpy as np

NC = 3
W = 4 * NC
T = 40
BANK_ROWS = (12, 25, 40)
MAX_PER_FRAME = 2


def make_bank(rows, nc, C, spf, seed, extra=3):
    """per class k: a waveform [C, rows[k] * spf + extra] of random floats and a label track [rows[k], 4*nc] with class k active in every row
    and a unit direction"""
    rng = np.random.default_rng(seed)
    tdm_x, tdm_y = [], []
    for k, r in enumerate(rows):
        tdm_x.append(rng.standard_normal((C, r * spf + extra)).astype(np.float32))
        lab = np.zeros((r, 4, nc), np.float32)
        d = rng.standard_normal((r, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        lab[:, 0, k] = 1
        lab[:, 1:, k] = d
        tdm_y.append(lab.reshape(r, 4 * nc))
    return tdm_x, tdm_y


def _labels(T, nc, active, seed, level=1.0):
    """active: {class: [(first frame, last frame + 1), ...]} -> [T, 4*nc]: activity `level` and a direction scaled by it"""
    rng = np.random.default_rng(seed)
    y = np.zeros((T, 4, nc), np.float32)
    for c, runs in active.items():
        for a, b in runs:
            d = rng.standard_normal((b - a, 3))
            d /= np.linalg.norm(d, axis=1, keepdims=True)
            y[a:b, 0, c] = level
            y[a:b, 1:, c] = d * level
    return y.reshape(T, 4 * nc)


def labels_case():
    """-> (y [3, 40, 12], plan int32 [3, 4, 4], expected valid vectors {(clip, k): list}).  B = 3, T = 40, nc = 3, K = 4, max_per_frame = 2, bank
    tracks of 12, 25 and 40 rows.  (cls, st, offset, td_offset):

    clip 0  class 0 active in frames 5-9, classes 1 and 2 in 10-14, class 1 in 30-34
      k0 (2, 5, 0, 0)     fully valid; offset = 0
      k1 (0, 10, 3, 2)    frames 3-4 valid, 5-9 class already active, 10-12 at max_per_frame; td_offset + st = bank_rows[0]
      k2 (1, 4, 2, 21)    overlaps k0 and k1: frame 2 valid, frames 3-4 at max_per_frame only because k0 and k1 both added there, frame 5
                          valid; td_offset + st = bank_rows[1]
      k3 (1, 3, 10, 0)    no valid frame
    clip 1  class 0 active in frames 36-39
      k0 (0, 1, 20, 5)    st = 1
      k1 (0, 6, 34, 0)    offset + st = T; frames 36-39 already active
      k2 (0, 6, 18, 3)    the same class again, across k0's frame 20: that frame is blocked by what k0 added
      k3 (2, 40, 0, 0)    the whole clip and the whole track, over every earlier insertion
    clip 2  fractional activities: class 0 at 0.5 in frames 0-19, class 1 at 0.5 in frames 10-29
      k0 (0, 8, 4, 1)     v = 0.5 everywhere
      k1 (1, 12, 8, 10)   v = 1 in frames 8-9, 0.5 in 10-19
      k2 (2, 5, 9, 30)    frames 9-11 reach 2.0 through k0 and k1 (blocked), 12-13 valid
      k3 (0, 2, 0, 0)     v = 0.5"""
    y = np.stack([
        _labels(T, NC, {0: [(5, 10)], 1: [(10, 15), (30, 35)], 2: [(10, 15)]}, 10),
        _labels(T, NC, {0: [(36, 40)]}, 11),
        _labels(T, NC, {0: [(0, 20)], 1: [(10, 30)]}, 12, level=0.5),
    ])
    plan = np.array([
        [[2, 5, 0, 0], [0, 10, 3, 2], [1, 4, 2, 21], [1, 3, 10, 0]],
        [[0, 1, 20, 5], [0, 6, 34, 0], [0, 6, 18, 3], [2, 40, 0, 0]],
        [[0, 8, 4, 1], [1, 12, 8, 10], [2, 5, 9, 30], [0, 2, 0, 0]],
    ], np.int32)
    expect = {
        (0, 0): [1] * 5, (0, 1): [1, 1] + [0] * 8, (0, 2): [1, 0, 0, 1], (0, 3): [0, 0, 0],
        (1, 0): [1], (1, 1): [1, 1, 0, 0, 0, 0], (1, 2): [1, 1, 0, 1, 1, 1],
        (1, 3): [1] * 40,      # the frames that hold class 0 (k0-k2, or from the start) hold one class: still below 2
        (2, 0): [0.5] * 8, (2, 1): [1, 1] + [0.5] * 10, (2, 2): [0, 0, 0, 1, 1], (2, 3): [0.5, 0.5],
    }
    return y, plan, expect


def long_case(seed=5):
    """more frames than a workgroup has threads: T = 320, st = 300.  -> (y [2, 320, 12], plan [2, 2, 4], bank rows)"""
    rows = (12, 320)
    y = np.stack([_labels(320, NC, {0: [(a, a + 7) for a in range(3, 300, 40)], 2: [(a, a + 11) for a in range(20, 310, 30)],
                                   1: [(a, a + 5) for a in range(25 + 3 * i, 300, 50)]}, seed + i) for i in range(2)])
    plan = np.array([[[1, 300, 10, 15], [0, 9, 100, 3]], [[1, 300, 20, 0], [1, 300, 0, 20]]], np.int32)
    return y, plan, rows


def waves(n, C, N, seed):
    return np.random.default_rng(seed).standard_normal((n, C, N)).astype(np.float32)
