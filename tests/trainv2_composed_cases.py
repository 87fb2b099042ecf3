"""Inputs and numpy restatements shared by tests/test_trainv2_composed_cpu.py and tests/test_trainv2_composed_gpu.py.  A helper, not a test
file."""
import numpy as np

import trainv2_oracle as V

# ---------------------------------------------------------------- the optimizer stage's variable table
# every rank the composed models hold: a conv kernel (rank 4), a vector, the GRU's (2, 384) bias, a head-major (H, D, dk) kernel, a
# depthwise (k, 1, C) kernel, a vector, a matrix that crosses the 4096-element segment boundary (1702 .. 5602), a short vector
OPT_SHAPES = [(3, 3, 4, 8), (13,), (2, 384), (4, 24, 6), (5, 1, 10), (7,), (130, 30), (3,)]
OPT_REG = [1, 0, 0, 1, 1, 0, 1, 0]
OPT_OFFSETS = [0, 288, 301, 1069, 1645, 1695, 1702, 5602]      # % 4 = 0, 0, 1, 1, 1, 3, 2, 2
OPT_N = 5605
OPT_SEED = 5


def rows_cols(shape):
    """utils.unitwise_norm's units as [rows][cols] (restated here: the library's own mapping is what test_unit_mapping checks)"""
    if len(shape) <= 1:
        return int(np.prod(shape)), 1
    if len(shape) in (2, 3):
        return shape[0], int(np.prod(shape[1:]))
    return int(np.prod(shape[:3])), shape[3]


def opt_weights(seed=OPT_SEED):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.standard_normal(int(np.prod(s))) * 0.2 for s in OPT_SHAPES]).astype(np.float32)


def opt_grads(th, step, seed=OPT_SEED):
    """tests/test_trainv2_gpu.py::_opt_grads on OPT_SHAPES: per unit of the CURRENT weights a gradient whose norm is 0.3 x or 3 x the unit's
    max_norm = max(|w_unit|, 1e-3) * 0.01, chosen at random.  The regulariser's 2 l2 w (l2 = 1e-3) moves a ratio by at most 0.2."""
    rng = np.random.default_rng(seed + 17 * step)
    g, off = [], 0
    for shape in OPT_SHAPES:
        rows, cols = rows_cols(shape)
        w = np.asarray(th[off:off + rows * cols], np.float64).reshape(rows, cols)
        d = rng.standard_normal((rows, cols))
        target = np.where(rng.random(cols) < 0.5, 0.3, 3.0) * np.maximum(np.linalg.norm(w, axis=0), 1e-3) * 0.01
        g.append((d * (target / np.linalg.norm(d, axis=0))).reshape(-1))
        off += rows * cols
    return np.concatenate(g).astype(np.float32)


def ratios_are_safe(r):
    """the oracle's grad_norm / max_norm lie on both sides of 1 and none within 1e-3 of it: no fp32 evaluation can flip a decision"""
    return bool((r < 1).any() and (r >= 1).any() and np.abs(r - 1).min() > 1e-3)


# ---------------------------------------------------------------- seld_aug_v2
def aug_v2_numpy(x, shift, n_shift_ch, tmask, fmask, period):
    """trainv2.get_dataset's sample transforms on a batch [B,T,F,C] (float32), restated: x[b, ..., :n_shift_ch] += shift[b]; then per sample
    and segment the frame runs and the bin runs become +0.  tmask / fmask: (size, offset) int [n][B * T/period], or None."""
    out = np.array(x, np.float32, copy=True)
    B, T, F, _ = out.shape
    nseg = T // period
    if shift is not None:
        out[..., :n_shift_ch] = out[..., :n_shift_ch] + np.asarray(shift, np.float32).reshape(B, 1, 1, 1)
    for b in range(B):
        for s in range(nseg):
            seg = out[b, s * period:(s + 1) * period]
            if tmask is not None:
                for size, off in zip(np.asarray(tmask[0])[:, b * nseg + s], np.asarray(tmask[1])[:, b * nseg + s]):
                    seg[off:off + size] = 0.0
            if fmask is not None:
                for size, off in zip(np.asarray(fmask[0])[:, b * nseg + s], np.asarray(fmask[1])[:, b * nseg + s]):
                    seg[:, off:off + size] = 0.0
    return out


def aug_draws(B, nseg, F, period, n_t, n_f, seed):
    """(shift, (t_size, t_off), (f_size, f_off)): random valid draws with hand-written entries on top — in column 0: a size 0, an offset 0,
    a run ending exactly at the segment's last frame and at the last bin, two overlapping runs; in the last column (when there is more than one): a bin run that covers
    the whole axis (every frame of that segment is fully masked) and a time run of the largest size"""
    rng = np.random.default_rng(seed)
    N = B * nseg
    shift = (rng.standard_normal(B) * 0.2).astype(np.float32)
    ts = rng.integers(0, 6, (n_t, N)).astype(np.int32)
    to = (rng.random((n_t, N)) * (period - ts)).astype(np.int32)
    fs = rng.integers(0, min(8, F), (n_f, N)).astype(np.int32)
    fo = (rng.random((n_f, N)) * (F - fs)).astype(np.int32)
    ts[0, 0], to[0, 0] = 0, 17                                # size 0: nothing
    ts[1, 0], to[1, 0] = 4, 0                                 # offset 0
    ts[2, 0], to[2, 0] = 5, period - 5                        # ends at the segment's last frame
    ts[3, 0], to[3, 0] = 5, 40                                # 40..44 and 43..47 overlap
    ts[4, 0], to[4, 0] = 5, 43
    fs[:, 0] = 0                                              # column 0's bin runs are all written here: bin F - 2 stays unmasked
    fs[0, 0], fo[0, 0] = 0, 1
    fs[1, 0], fo[1, 0] = 1, 0
    fs[2, 0], fo[2, 0] = 1, F - 1                             # ends at the last bin
    fs[3, 0], fo[3, 0] = 2, 1                                 # 1..2 and 2 overlap
    fs[4, 0], fo[4, 0] = 1, 2
    if N > 1:
        fs[5, N - 1], fo[5, N - 1] = F, 0                     # the whole axis
        ts[5, N - 1], to[5, N - 1] = 5, 50
    assert (to + ts <= period).all() and (fo + fs <= F).all()
    return shift, (ts, to), (fs, fo)


def swa_numpy(swa, w, cnt):
    return V.swa_update(swa, w, cnt)
