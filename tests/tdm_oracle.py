"""Numpy restatement of the reference's data_loader.TDM_aug (data_loader.py:188-234) given an explicit plan.  TEST INFRASTRUCTURE ONLY.

The reference draws (cls, sample_time, offset, td_offset) per insertion with TensorFlow's generator; here they arrive as a plan
int [n, K, 4] = (cls, st, offset, td_offset), and everything behind the draws is restated in float32, in the reference's order:

    frame_y     = y[i][offset : offset + st]
    valid_index = float(sum(frame_y[:, :nc], -1) < max_overlap_per_frame) * (1 - frame_y[:, cls])      the sum over c ascending
    if sum(valid_index) == 0: nothing is added
    y[i] += pad(tdm_y[cls][td : td + st] * valid_index[:, None])
    x[i] += pad(tdm_x[cls][:, td * spf : (td + st) * spf] * repeat(valid_index, spf)[None])

one insertion after the other, so a later insertion sees the labels the earlier ones left.  The pad's zeros change no finite sample
(x + 0 = x), so the adds are restated on the slice the insertion covers.  Also returned: the valid_index vectors, as float32
[n, K, max(1, longest st)], zero behind st, which is what seld_aug_tdm_labels writes.
"""
import numpy as np


def valid_index(frame_y, cls, nc, max_per_frame):
    s = np.zeros(frame_y.shape[0], np.float32)
    for c in range(nc):
        s = (s + frame_y[:, c]).astype(np.float32)
    return ((s < np.float32(max_per_frame)).astype(np.float32) * (np.float32(1) - frame_y[:, cls])).astype(np.float32)


def tdm_aug(x, y, tdm_x, tdm_y, plan, spf, max_per_frame=2):
    """x [n, C, N], y [n, T, 4*nc] (float32 arrays, not modified), the bank as lists of [C, n_k] and [t_k, 4*nc], plan int [n, K, 4]
    -> (x', y', valid)."""
    x = np.array(x, np.float32, copy=True)
    y = np.array(y, np.float32, copy=True)
    plan = np.asarray(plan).astype(np.int64)
    n, K = plan.shape[:2]
    nc = y.shape[-1] // 4
    ld = max(1, int(plan[..., 1].max())) if plan.size else 1
    valid = np.zeros((n, K, ld), np.float32)
    for i in range(n):
        for k in range(K):
            cls, st, off, td = (int(v) for v in plan[i, k])
            if st == 0:
                continue
            assert 0 <= cls < len(tdm_y) and st > 0 and off >= 0 and off + st <= y.shape[1] and td >= 0 and td + st <= tdm_y[cls].shape[0]
            v = valid_index(y[i, off:off + st], cls, nc, max_per_frame)
            valid[i, k, :st] = v
            if v.sum() == 0:
                continue
            ty = (np.asarray(tdm_y[cls], np.float32)[td:td + st] * v[:, None]).astype(np.float32)
            y[i, off:off + st] = (y[i, off:off + st] + ty).astype(np.float32)
            tx = (np.asarray(tdm_x[cls], np.float32)[:, td * spf:(td + st) * spf] * np.repeat(v, spf)[None]).astype(np.float32)
            x[i, :, off * spf:(off + st) * spf] = (x[i, :, off * spf:(off + st) * spf] + tx).astype(np.float32)
    return x, y, valid
