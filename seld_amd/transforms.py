"""Mirror of the reference's transforms.py for the accelerated path: the batch augmentations of train.get_dataset
(train.py:157-165) on DEVICE tensors through the C ABI (seld_aug_mask, seld_aug_gather_sign), plus the pure index
helpers.  Randomness: the reference draws with tf.random.uniform inside tf.data; here a numpy Generator makes the
same draws on the host (same distributions: size ~ U{0..max_mask_size-1}, offset ~ U{0..total-size-1},
flip ~ U{0,1}^3, swap ~ U{0,2}, acs index ~ U{0..7}) and only the small tables go to the device.

  mask(specs, axis, max_mask_size, period, n_mask, rng)   transforms.py:6-44    specs [B,T,F,C] batch (each sample and
                                                                               each period-frame segment its own draw)
  foa_intensity_vec_aug(x, y, rng)                         transforms.py:73-114
  acs_aug(x, y, rng)                                       transforms.py:159-207
  mic_gcc_perm(mic_perm)                                   transforms.py:122-140
  split_total_labels_to_sed_doa(x, y)                      transforms.py:117-119
  random_ups_and_downs(x, rng)                             trainv2.py:120-124   one N(0, 0.2^2) shift per sample on the first 4 channels
  v2_sample_transforms(x, rng, time, freq, period)         trainv2.py:133-140   that shift, 10 time masks and 6 frequency masks in ONE
                                                                               pass (seld_aug_v2)
  mcs_aug(iteration, theta)(x, y)                           transforms.py:202-291   CGMM mask estimation in float64, one kernel for the whole
                                                                               function (seld_aug_mcs); mcs_mask returns the mask itself"""
from __future__ import annotations

import collections
import ctypes as C

import numpy as np
import torch

from . import _lib

# transforms.py:146-155
channel_list = [
    [[1, 3, 0, 2], [0, -3, -2, 1]],
    [[3, 1, 2, 0], [0, -3, 2, -1]],
    [[0, 1, 2, 3], [0, 1, 2, 3]],
    [[1, 0, 3, 2], [0, -1, -2, 3]],
    [[2, 0, 3, 1], [0, 3, -2, -1]],
    [[0, 2, 1, 3], [0, 3, 2, 1]],
    [[3, 2, 1, 0], [0, -1, 2, -3]],
    [[2, 3, 0, 1], [0, 1, -2, -3]],
]


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev_tensor(x, name):
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()):
        raise ValueError(f"{name} must be a contiguous float32 CUDA tensor (augmentation runs on the device)")
    return x


def split_total_labels_to_sed_doa(x, y):
    n_classes = y.shape[-1] // 4
    return x, (y[..., :n_classes], y[..., n_classes:])


def draw_mask(rng, n, total, max_mask_size):
    """(size, offset) int32 [n]: tf.random.uniform([], maxval=max_mask_size) and ([], maxval=total - size)."""
    if max_mask_size is None:
        max_mask_size = total
    size = rng.integers(0, max_mask_size, size=n)
    if (total - size <= 0).any():
        raise ValueError("max_mask_size must be smaller than the masked axis")      # tf.random.uniform(maxval=0) fails too
    offset = (rng.random(n) * (total - size)).astype(np.int64)
    return size.astype(np.int32), offset.astype(np.int32)


def mask(specs, axis, max_mask_size=None, period=100, n_mask=1, rng=None, draws=None):
    """In-place on specs [B,T,F,C] (device).  axis: -3 (time) or -2 (frequency), as in the reference's per-sample call
    (there specs is [T,F,C]).  `draws` = (size, offset) int arrays [B * T//period] overrides the generator (tests)."""
    specs = _dev_tensor(specs, "specs")
    if specs.dim() != 4 or axis not in (-3, -2):
        raise ValueError("mask: specs must be [B,T,F,C] and axis -3 or -2")
    B, T, F, Cc = specs.shape
    if T % period != 0:
        raise ValueError("(spec time length / period)' rest must be 0")
    lib = _lib.load()
    nseg = T // period
    total = period if axis == -3 else F
    rng = rng or np.random.default_rng()
    for _ in range(n_mask):
        size, offset = draws if draws is not None else draw_mask(rng, B * nseg, total, max_mask_size)
        sz = torch.as_tensor(np.ascontiguousarray(size, np.int32)).to(specs.device)
        of = torch.as_tensor(np.ascontiguousarray(offset, np.int32)).to(specs.device)
        args = (_ptr(of), _ptr(sz), None, None) if axis == -3 else (None, None, _ptr(of), _ptr(sz))
        rc = lib.seld_aug_mask(_ptr(specs), B, T, F, Cc, period, *args, _stream())
        if rc:
            raise _lib.SeldError(f"seld_aug_mask failed ({rc})")
    return specs


# seld_aug_v2 reads its tables where the host wrote them (pinned memory): they stay alive here until the kernel that reads them has run
_v2_in_flight = collections.deque()
UPS_AND_DOWNS_CHANNELS = 4      # trainv2.py:122: x[..., :4]
UPS_AND_DOWNS_STDDEV = 0.2


def _pinned(a, dtype):
    """a host array -> a pinned tensor the device can read (one host copy)"""
    a = np.ascontiguousarray(a, dtype)
    t = torch.empty(a.shape, dtype=torch.float32 if dtype == np.float32 else torch.int32, pin_memory=True)
    t.numpy()[...] = a
    return t


def draw_v2(rng, B, nseg, F, time=(6, 10), freq=(8, 6), period=100):
    """the draws of one batch: (shift float32 [B], (t_size, t_off) int32 [n_t][B * nseg] each, (f_size, f_off) [n_f][B * nseg] each)"""
    shift = (rng.standard_normal(B) * UPS_AND_DOWNS_STDDEV).astype(np.float32)
    tm = [draw_mask(rng, B * nseg, period, time[0]) for _ in range(time[1])]
    fm = [draw_mask(rng, B * nseg, F, freq[0]) for _ in range(freq[1])]
    pack = lambda m, k: np.stack([d[k] for d in m]).astype(np.int32) if m else np.zeros((0, B * nseg), np.int32)
    return shift, (pack(tm, 0), pack(tm, 1)), (pack(fm, 0), pack(fm, 1))


def _aug_v2(x, shift, tmask, fmask, period):
    x = _dev_tensor(x, "x")
    if x.dim() != 4:
        raise ValueError("x must be [B,T,F,C]")
    B, T, F, Cc = x.shape
    if T % period != 0:
        raise ValueError("(spec time length / period)' rest must be 0")
    N = B * (T // period)
    keep, args = [], []
    if shift is not None:
        sh = _pinned(np.asarray(shift).reshape(B), np.float32)
        keep.append(sh)
    for m in (tmask, fmask):
        size, off = (np.asarray(a).reshape(-1, N) for a in m) if m is not None else (np.zeros((0, N)), np.zeros((0, N)))
        n = size.shape[0]
        if n:
            tab = _pinned(np.stack([off, size]), np.int32)       # [2][n][N]: one copy per axis
            keep.append(tab)
            args += [C.c_void_p(tab[0].data_ptr()), C.c_void_p(tab[1].data_ptr()), n]
        else:
            args += [None, None, 0]
    rc = _lib.load().seld_aug_v2(_ptr(x), B, T, F, Cc, period, _ptr(sh) if shift is not None else None, min(UPS_AND_DOWNS_CHANNELS, Cc), *args,
                                 _stream())
    if rc:
        raise _lib.SeldError(rc, "seld_aug_v2 refused its arguments")
    while _v2_in_flight and _v2_in_flight[0][0].query():
        _v2_in_flight.popleft()
    if keep:
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(x.device))
        _v2_in_flight.append((ev, keep))
    return x


def random_ups_and_downs(x, rng=None, draws=None):
    """trainv2.random_ups_and_downs (trainv2.py:120-124) on a device batch [B,T,F,C], in place: one N(0, 0.2^2) float32 per sample added to
    the first 4 channels.  `draws` = shift [B] overrides the generator (tests)."""
    rng = rng or np.random.default_rng()
    shift = draws if draws is not None else (rng.standard_normal(x.shape[0]) * UPS_AND_DOWNS_STDDEV).astype(np.float32)
    return _aug_v2(x, shift, None, None, int(x.shape[1]))      # no masks: one segment per sample


def v2_sample_transforms(x, rng=None, draws=None, time=(6, 10), freq=(8, 6), period=100):
    """trainv2.get_dataset's sample transforms (trainv2.py:133-140) on a device batch [B,T,F,C], in place, in one kernel: random_ups_and_downs,
    then mask(axis=-3, max_mask_size=time[0], n_mask=time[1]) and mask(axis=-2, max_mask_size=freq[0], n_mask=freq[1]).  The host makes the
    draws (draw_v2) and writes three tables: the shifts, the time runs, the frequency runs.  `draws` = what draw_v2 returns (tests)."""
    if x.dim() != 4 or x.shape[1] % period != 0:
        raise ValueError("x must be [B,T,F,C] with (spec time length / period)' rest 0")
    B, T, F, _ = x.shape
    rng = rng or np.random.default_rng()
    shift, tmask, fmask = draws if draws is not None else draw_v2(rng, B, T // period, F, time, freq, period)
    return _aug_v2(x, shift, tmask, fmask, period)


def _gather_sign(t, B, outer, R, inner, src, sgn):
    lib = _lib.load()
    s = torch.as_tensor(np.ascontiguousarray(src, np.int32)).to(t.device)
    g = torch.as_tensor(np.ascontiguousarray(sgn, np.float32)).to(t.device)
    rc = lib.seld_aug_gather_sign(_ptr(t), B, outer, R, inner, _ptr(s), _ptr(g), _stream())
    if rc:
        raise _lib.SeldError(f"seld_aug_gather_sign failed ({rc})")


def foa_tables(flip, p):
    """src/sgn tables of foa_intensity_vec_aug for x (7 channels) and y rows (4): transforms.py:88-111."""
    flip, p = np.asarray(flip), np.asarray(p).reshape(-1)
    B = flip.shape[0]
    s = 1 - 2 * flip.astype(np.int64)                                   # sign per ORIGINAL axis, applied before the gather
    perm = np.stack([p, np.ones_like(p), 2 - p], -1)
    check = (perm != np.array([[0, 1, 2]])).sum(-1, keepdims=True)
    fp = (perm + check) % 3
    b = np.arange(B)[:, None]
    x_src = np.concatenate([np.zeros((B, 1), np.int64), 1 + perm, 4 + fp], -1)
    x_sgn = np.concatenate([np.ones((B, 4)), s[b, fp]], -1)
    y_src = np.concatenate([np.zeros((B, 1), np.int64), 1 + fp], -1)
    y_sgn = np.concatenate([np.ones((B, 1)), s[b, fp]], -1)
    return x_src, x_sgn, y_src, y_sgn


def foa_intensity_vec_aug(x, y, rng=None, draws=None):
    """x [B,T,F,7], y [B,S,4*n_classes] device tensors, modified in place and returned.  `draws` = (flip [B,3], p [B])."""
    x, y = _dev_tensor(x, "x"), _dev_tensor(y, "y")
    B, T, F, Cc = x.shape
    if Cc != 7:
        raise ValueError("foa_intensity_vec_aug expects 7 feature channels")
    rng = rng or np.random.default_rng()
    flip, p = draws if draws is not None else (rng.integers(0, 2, (B, 3)), 2 * rng.integers(0, 2, B))
    x_src, x_sgn, y_src, y_sgn = foa_tables(flip, p)
    _gather_sign(x, B, T * F, 7, 1, x_src, x_sgn)
    nc = y.shape[-1] // 4
    _gather_sign(y, B, int(np.prod(y.shape[1:-1])), 4, nc, y_src, y_sgn)
    return x, y


def mic_gcc_perm(mic_perm):
    pairs = np.array([[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]])
    mic_perm = np.asarray(mic_perm)
    order = {(a, b): k for k, (a, b) in enumerate(pairs.tolist())}
    out = np.empty((mic_perm.shape[0], 6), np.int64)
    for k, (a, b) in enumerate(pairs.tolist()):
        for i in range(mic_perm.shape[0]):
            u, v = int(mic_perm[i, a]), int(mic_perm[i, b])
            out[i, k] = order[(min(u, v), max(u, v))]
    return out


def acs_tables(idx):
    """src/sgn tables of acs_aug for x (17 channels) and y rows (4): transforms.py:175-203."""
    cl = np.array(channel_list)[np.asarray(idx)]
    B = cl.shape[0]
    foa_flip = cl[:, 1, 1:]
    sgn = np.sign(foa_flip)
    foa_perm = sgn * foa_flip - 1
    check = (foa_perm != np.array([0, 1, 2])).sum(-1, keepdims=True)
    fp = (foa_perm + check) % 3
    mic = cl[:, 0, :]
    x_src = np.concatenate([np.zeros((B, 1), np.int64), 1 + foa_perm, 4 + fp, 7 + mic, 11 + mic_gcc_perm(mic)], -1)
    x_sgn = np.concatenate([np.ones((B, 4)), sgn, np.ones((B, 10))], -1)           # sign indexed by OUTPUT position
    y_src = np.concatenate([np.zeros((B, 1), np.int64), 1 + fp], -1)
    y_sgn = np.concatenate([np.ones((B, 1)), sgn], -1)
    return x_src, x_sgn, y_src, y_sgn


def acs_aug(x, y, rng=None, draws=None):
    """x [B,T,F,17] (foa 4, intensity 3, mic 4, gcc 6), y [B,S,4*n_classes]; in place.  `draws` = idx [B] in [0,8)."""
    x, y = _dev_tensor(x, "x"), _dev_tensor(y, "y")
    B, T, F, Cc = x.shape
    if Cc != 17:
        raise ValueError("acs_aug expects 17 feature channels")
    rng = rng or np.random.default_rng()
    idx = draws if draws is not None else rng.integers(0, 8, B)
    x_src, x_sgn, y_src, y_sgn = acs_tables(idx)
    _gather_sign(x, B, T * F, 17, 1, x_src, x_sgn)
    nc = y.shape[-1] // 4
    _gather_sign(y, B, int(np.prod(y.shape[1:-1])), 4, nc, y_src, y_sgn)
    return x, y


def _mcs_input(x):
    """the shape the kernel holds on chip, judged by the library before the tensor itself is"""
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise ValueError("mcs_aug: x must be a [B,T,F,C] tensor")
    max_frames = _lib.load().seld_aug_mcs_max_frames(int(x.shape[3]))
    if max_frames == 0 or x.shape[1] > max_frames:
        raise ValueError(f"mcs_aug: x {tuple(x.shape)}: 1..10 channels" + (f" and at most {max_frames} frames" if max_frames else ""))
    return _dev_tensor(x, "x")


def _mcs(x, out, lam, adds, iteration, theta):
    B, T, F, Cc = x.shape
    rc = _lib.load().seld_aug_mcs(_ptr(x), _ptr(out), _ptr(lam), _ptr(adds), B, T, F, Cc, int(iteration), float(theta), _stream())
    if rc in (-1, -2):
        raise ValueError(f"mcs_aug: {_lib.ERR_NAMES[rc]} for x {tuple(x.shape)}, iteration {iteration}, theta {theta}: needs iteration >= 1, a finite "
                         f"theta >= 0, 1..10 channels and at most seld_aug_mcs_max_frames(C) frames")
    if rc:
        raise _lib.SeldError(rc, "seld_aug_mcs failed")


def mcs_aug(iteration: int, theta=1e-6):
    """transforms.mcs_aug (transforms.py:231-291): _mcs_aug(x, y) -> (x, y) multiplies x [B,T,F,C] (device), in place, by the noise mask of a
    two-class complex-Gaussian mixture model fitted per (sample, frequency bin) in float64 over `iteration` EM rounds; y is returned untouched."""
    if int(iteration) < 1:
        raise ValueError("mcs_aug: iteration must be at least 1 (the reference's function has no result otherwise)")

    def _mcs_aug(x, y):
        _mcs(_mcs_input(x), x, None, None, iteration, theta)
        return x, y
    return _mcs_aug


def mcs_mask(x, iteration, theta=1e-6):
    """-> (lambda_noise [B,T,F] float64, stab_adds [B,F,2,iteration+1] int32: the diagonal additions of every stab call, class noisy then class
    noise, the initialisation's call first).  x [B,T,F,C] (device) is left alone."""
    if int(iteration) < 1:
        raise ValueError("mcs_mask: iteration must be at least 1")
    x = _mcs_input(x)
    B, T, F, _ = x.shape
    out = torch.empty_like(x)
    lam = torch.empty((B, T, F), dtype=torch.float64, device=x.device)
    adds = torch.empty((B, F, 2, int(iteration) + 1), dtype=torch.int32, device=x.device)
    _mcs(x, out, lam, adds, iteration, theta)
    return lam, adds
