"""Data boundary of the reference, host side (numpy): the `.npy` dataset layout, fold selection and
windowing of data_loader.py, without tf.data.

  load_seldnet_data            data_loader.py:58-92   glob *.npy, fold = 5th character of the file name
  seldnet_data_to_dataloader   data_loader.py:132-168 + data_loader():13-55
      concat files -> [labels, 5, F, C] -> windows of 60 labels (300 frames) -> repeat(loop_time) ->
      batch(batch_size, drop_remainder=False) -> [device_transforms: augmentation on the device batch, run by
      the step loop] -> split labels into (sed, doa) -> shuffle (train)
Batches are (x [b,300,F,C] float32, (sed [b,60,C], doa [b,60,3C])) numpy arrays; pinned host buffers
and the H2D copy belong to the caller (`train.trainstep` accepts numpy or device tensors).

Time-domain mixing (what train.get_tdm_dataset regenerates the training set with):
  load_wav_and_label           data_loader.py:95-129   *.wav + metadata *.csv of one split -> ([4, n] float32 waves, [600, 4*nc] labels)
  get_TDMset                   data_loader.py:171-185  the bank of single-class clips: per class a waveform [4, n_k] and a label track [t_k, 4*nc]
  draw_tdm                     data_loader.py:201-209  the draws of TDM_aug as a plan int32 [n, K, 4] = (cls, st, offset, td_offset)
  TdmBank                      the bank packed on the device once (seld_hip.h: seld_aug_tdm_*), reused by every regeneration
  TDM_aug                      data_loader.py:188-234  on DEVICE tensors: seld_aug_tdm_labels, then seld_aug_tdm_mix
Deviations from the reference, all at the boundary: TensorFlow's generator is replaced by `rng` (a numpy Generator making the same draws:
class ~ categorical(1 / track length), st ~ U[min, max), offset ~ U[0, T - st), td_offset ~ U[0, t_cls - st)) or by an explicit plan `draws`;
the bank is read from .npy files, not .joblib (no joblib here); wav files are read with the standard `wave` module (16-bit PCM, scaled by
1 / 32768 as tf.audio.decode_wav does); n_classes is a parameter instead of the 14 extract_labels defaults to."""
from __future__ import annotations

import ctypes as C
import os
import wave
from glob import glob

import numpy as np

from .feature_extractor import extract_labels

SPLITS = {'train': [1, 2, 3, 4], 'val': [5], 'test': [6]}
TDM_MAX_INSERTIONS = 32      # seld_aug_tdm_*: insertions per clip


def load_seldnet_data(feat_path, label_path, mode='train', n_freq_bins=64):
    assert mode in SPLITS
    out = []
    for path, what in ((feat_path, 'feat_path'), (label_path, 'label_path')):
        if not os.path.exists(path):
            raise ValueError(f'no such {what} ({path}) exists')
        files = sorted(glob(os.path.join(path, '*.npy')))
        out.append([np.load(f).astype('float32') for f in files
                    if int(f[f.rfind(os.path.sep) + 5]) in SPLITS[mode]])
    features, labels = out
    if features and features[0].ndim == 2:
        features = [np.reshape(x, (x.shape[0], -1, n_freq_bins)).transpose(0, 2, 1) for x in features]
    return features, labels


def split_total_labels_to_sed_doa(x, y):
    """transforms.py:117-119"""
    n_classes = y.shape[-1] // 4
    return x, (y[..., :n_classes], y[..., n_classes:])


class SeldDataset:
    """Iterable of batches with the structure the reference's tf.data pipeline yields."""

    def __init__(self, x, y, batch_size, train, loop_time, shuffle_size, seed=None, device_transforms=None):
        self.x, self.y = x, y
        self.batch_size, self.train, self.loop_time, self.shuffle_size = batch_size, train, loop_time, shuffle_size
        self.rng = np.random.default_rng(seed)
        # augmentations f(x_dev, y_total_dev, rng) -> (x_dev, y_total_dev) run by the step loop on the device batch
        # (seld_amd.transforms); with any of them the labels stay unsplit until they have run
        self.device_transforms = list(device_transforms or [])

    def to_device(self, device):
        """Keep the whole windowed dataset resident in HBM (DCASE dev set: 600 clips x 5.4 MB = 3.2 GB of 288 GB): a
        batch is then a device-side row gather and no byte crosses PCIe per step.  Batches become torch tensors."""
        import torch
        self.x = torch.as_tensor(self.x).to(device)
        self.y = torch.as_tensor(self.y).to(device)
        return self

    def __len__(self):
        n = self.x.shape[0] * (self.loop_time if self.train else 1)
        return -(-n // self.batch_size)

    def _batches(self):
        reps = self.loop_time if self.train else 1
        idx = np.concatenate([np.arange(self.x.shape[0])] * reps)      # cache().repeat(loop_time)
        for i in range(0, idx.size, self.batch_size):                  # batch(drop_remainder=False)
            sel = idx[i:i + self.batch_size]
            if not isinstance(self.x, np.ndarray):                     # HBM-resident: gather on the device
                import torch
                sel = torch.as_tensor(sel, device=self.x.device)
            if self.device_transforms:
                yield self.x[sel], self.y[sel]                         # total labels [b,60,4C]: split after the transforms
            else:
                yield split_total_labels_to_sed_doa(self.x[sel], self.y[sel])

    def __iter__(self):
        if not self.train or not self.shuffle_size or self.shuffle_size <= 1:
            yield from self._batches()
            return
        buf = []                                                       # tf.data shuffle(buffer) of BATCHES
        for b in self._batches():
            buf.append(b)
            if len(buf) >= self.shuffle_size:
                yield buf.pop(int(self.rng.integers(len(buf))))
        while buf:
            yield buf.pop(int(self.rng.integers(len(buf))))

    def take(self, n):
        for i, b in enumerate(self):
            if i >= n:
                break
            yield b


def seldnet_data_to_dataloader(features, labels, train=True, label_window_size=60, drop_remainder=True,
                               shuffle_size=None, batch_size=32, loop_time=1, seed=None, **kwargs):
    if kwargs.get('sample_transforms') or kwargs.get('preprocessing') or kwargs.get('batch_transforms'):
        raise ValueError('host-side tf.data transforms are not taken: pass device_transforms (seld_amd.transforms)')
    device_transforms = kwargs.get('device_transforms')
    total_length = labels[0].shape[0]
    features = np.concatenate(features, axis=0)
    labels = np.concatenate(labels, axis=0)
    features = np.reshape(features, (labels.shape[0], -1, *features.shape[1:]))    # [labels, 5, F, C]
    n_samples = features.shape[0] // label_window_size
    if not drop_remainder and features.shape[0] % label_window_size:
        raise ValueError('drop_remainder=False with a ragged last window is not supported')
    x = features[:n_samples * label_window_size].reshape(n_samples, -1, *features.shape[2:])
    y = labels[:n_samples * label_window_size].reshape(n_samples, label_window_size, -1)
    if not train:
        batch_size = total_length // label_window_size          # one file per batch (data_loader.py:157-158)
    if train and shuffle_size is None:
        shuffle_size = n_samples // batch_size
    return SeldDataset(np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32), batch_size, train,
                       loop_time, shuffle_size, seed, device_transforms)


# ---------------------------------------------------------------------------------------------------
# time-domain mixing (data_loader.py:95-129, 171-234)
def _fold_of(path):
    return int(path[path.rfind(os.path.sep) + 5])


def _read_wav(path):
    """-> float32 [channels, n]: 16-bit PCM scaled by 1 / 32768 (tf.audio.decode_wav), transposed as data_loader.py:127 does"""
    with wave.open(path, 'rb') as w:
        if w.getsampwidth() != 2 or w.getcomptype() != 'NONE':
            raise ValueError(f'{path}: only 16-bit PCM wav files are read')
        ch, n = w.getnchannels(), w.getnframes()
        pcm = np.frombuffer(w.readframes(n), dtype='<i2').reshape(-1, ch)
    return np.ascontiguousarray(pcm.T).astype(np.float32) * np.float32(1.0 / 32768.0)


def load_wav_and_label(feat_path, label_path, mode='train', n_classes=14, max_label_length=600):
    """reference data_loader.load_wav_and_label (data_loader.py:95-129) -> (x: list of float32 [4, n], y: list of float32
    [max_label_length, 4 * n_classes]); files selected by the fold digit of their name, as load_seldnet_data does."""
    assert mode in SPLITS
    f_paths = [f for f in sorted(glob(os.path.join(feat_path, '*.wav'))) if _fold_of(f) in SPLITS[mode]]
    l_paths = [f for f in sorted(glob(os.path.join(label_path, '*.csv'))) if _fold_of(f) in SPLITS[mode]]
    if len(f_paths) != len(l_paths):
        raise ValueError('# of features and labels are not matched')

    def preprocess_label(labels):
        if labels.shape[0] < max_label_length:
            return np.pad(labels, ((0, max_label_length - labels.shape[0]), (0, 0)))
        return labels[:max_label_length]
    x = [_read_wav(f) for f in f_paths]
    y = [preprocess_label(extract_labels(f, n_classes=n_classes)) for f in l_paths]
    return x, y


def get_TDMset(TDM_PATH, sr=24000, label_resolution=0.1):
    """reference data_loader.get_TDMset (data_loader.py:171-185) -> (tdm_x: list of float32 [4, n_k], tdm_y: list of float32 [t_k, 4*nc]) read from
    TDM_PATH/foa_dev_tdm/tdm_noise_{k}.npy and tdm_label_{k}.npy (.npy, not the reference's .joblib).  A waveform shorter than its label
    track (n_k < t_k * samples per label frame) is refused: TDM_aug would slice behind its end."""
    tdm_path = os.path.join(TDM_PATH, 'foa_dev_tdm')
    class_num = len(glob(os.path.join(tdm_path, '*label_*.npy')))
    spf = int(sr * label_resolution)
    tdm_x, tdm_y = [], []
    for k in range(class_num):
        wav = np.load(os.path.join(tdm_path, f'tdm_noise_{k}.npy')).astype(np.float32)
        lab = np.load(os.path.join(tdm_path, f'tdm_label_{k}.npy')).astype(np.float32)
        if wav.ndim != 2 or lab.ndim != 2 or lab.shape[1] % 4:
            raise ValueError(f'tdm class {k}: the waveform must be [channels, n] and the labels [t, 4 * n_classes]')
        if wav.shape[1] < lab.shape[0] * spf:
            raise ValueError(f'tdm class {k}: {wav.shape[1]} samples are fewer than {lab.shape[0]} label frames of {spf} samples')
        tdm_x.append(wav)
        tdm_y.append(lab)
    return tdm_x, tdm_y


def tdm_frames(sec, label_resolution=0.1):
    """seconds -> label frames as data_loader.py:196-197 does it: int() of the float quotient, not rounded (0.3 / 0.1 -> 2, 0.5 / 0.1 -> 5)"""
    return int(sec / label_resolution)


def draw_tdm(rng, n_clips, T, bank_rows, K, min_frames, max_frames):
    """The draws of TDM_aug (data_loader.py:201-209) for n_clips clips of T label frames -> plan int32 [n_clips, K, 4] = (cls, st, offset,
    td_offset): K classes per clip with replacement, p ~ 1 / bank_rows; per insertion st ~ U[min_frames, max_frames), offset ~ U[0, T - st),
    td_offset ~ U[0, bank_rows[cls] - st).  ValueError where tf.random.uniform would be given maxval <= minval."""
    rows = np.asarray(bank_rows, np.int64).reshape(-1)
    if rows.size == 0 or (rows < 1).any():
        raise ValueError('draw_tdm: every class of the bank needs at least one label frame')
    if K < 0 or K > TDM_MAX_INSERTIONS:
        raise ValueError(f'draw_tdm: 0..{TDM_MAX_INSERTIONS} insertions per clip')
    if max_frames <= min_frames or min_frames < 0:
        raise ValueError(f'draw_tdm: the insertion length is drawn from [{min_frames}, {max_frames}): empty')
    if T - (max_frames - 1) <= 0:
        raise ValueError(f'draw_tdm: an insertion of {max_frames - 1} frames leaves no offset in a clip of {T}')
    if (rows - (max_frames - 1) <= 0).any():
        raise ValueError(f'draw_tdm: an insertion of {max_frames - 1} frames leaves no offset in the shortest bank track ({int(rows.min())})')
    w = 1.0 / rows
    w /= w.sum()
    cls = rng.choice(rows.size, size=(n_clips, K), p=w)
    st = rng.integers(min_frames, max_frames, size=(n_clips, K))
    offset = rng.integers(0, T - st)
    td = rng.integers(0, rows[cls] - st)
    return np.stack([cls, st, offset, td], axis=-1).astype(np.int32)


def check_tdm_draws(draws, n_clips, T, bank_rows):
    """-> the plan as a contiguous int32 [n_clips, K, 4] array; ValueError for a wrong dtype or shape, or a row that reaches outside the clip or
    its class's track (the kernels skip such a row; here it is the caller's mistake)."""
    d = np.asarray(draws)
    if d.dtype.kind not in 'iu':
        raise ValueError(f'draws must be integers, not {d.dtype}')
    if d.ndim != 3 or d.shape[0] != n_clips or d.shape[2] != 4:
        raise ValueError(f'draws must be [{n_clips}, K, 4] = (cls, st, offset, td_offset), not {d.shape}')
    if d.shape[1] > TDM_MAX_INSERTIONS:
        raise ValueError(f'draws: at most {TDM_MAX_INSERTIONS} insertions per clip')
    rows = np.asarray(bank_rows, np.int64).reshape(-1)
    d = d.astype(np.int64)
    cls, st, off, td = d[..., 0], d[..., 1], d[..., 2], d[..., 3]
    if ((cls < 0) | (cls >= rows.size)).any():
        raise ValueError(f'draws: class outside [0, {rows.size})')
    if ((st < 0) | (off < 0) | (off + st > T)).any():
        raise ValueError(f'draws: an insertion reaches outside the clip of {T} label frames')
    if ((td < 0) | (td + st > rows[cls])).any():
        raise ValueError("draws: an insertion reaches outside its class's bank track")
    return np.ascontiguousarray(d, np.int32)


class TdmBank:
    """The bank of get_TDMset packed on the device once, in the layout seld_aug_tdm_labels / seld_aug_tdm_mix read (include/seld_hip.h): the label
    tracks row-wise in one [sum t_k, 4*nc] tensor, the waveforms as blocks [C][n_k] one behind the other (n_k trimmed to the track's
    t_k * spf samples, which is all TDM_aug can reach, and a multiple of 4 when spf is)."""

    def __init__(self, tdm_x, tdm_y, sr=24000, label_resolution=0.1, device=None):
        import torch
        if len(tdm_x) != len(tdm_y) or len(tdm_y) == 0:
            raise ValueError('the bank needs one waveform and one label track per class')
        self.spf = int(sr * label_resolution)
        self.rows = np.array([int(t.shape[0]) for t in tdm_y], np.int64)
        self.W = int(tdm_y[0].shape[1])
        self.C = int(tdm_x[0].shape[0])
        for k, (wv, lb) in enumerate(zip(tdm_x, tdm_y)):
            if lb.shape[1] != self.W or wv.shape[0] != self.C:
                raise ValueError(f'tdm class {k}: every class needs the same channels and label width')
            if wv.shape[1] < lb.shape[0] * self.spf:
                raise ValueError(f'tdm class {k}: {wv.shape[1]} samples are fewer than {lb.shape[0]} label frames of {self.spf} samples')
        if not torch.cuda.is_available():
            from . import _lib
            raise _lib.SeldLibraryError('no HIP device visible: seld_amd has no CPU fallback')
        dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        as_t = lambda a: (a.detach() if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))).to(dev, torch.float32)
        n_k = self.rows * self.spf
        self.s0 = np.concatenate([[0], np.cumsum(n_k * self.C)]).astype(np.int64)
        self.row0 = np.concatenate([[0], np.cumsum(self.rows)[:-1]]).astype(np.int64)
        self.bank_x = torch.cat([as_t(wv)[:, :int(n)].reshape(-1) for wv, n in zip(tdm_x, n_k)]).to(dev)
        self.bank_y = torch.cat([as_t(lb) for lb in tdm_y]).contiguous().to(dev)
        self.d_s0 = torch.as_tensor(self.s0).to(dev)
        self.d_row0 = torch.as_tensor(self.row0).to(dev)
        self.d_rows = torch.as_tensor(self.rows).to(dev)
        self.device = dev


def _tdm_bank_rows(tdm_x, tdm_y):
    return tdm_x.rows if isinstance(tdm_x, TdmBank) else np.array([int(t.shape[0]) for t in tdm_y], np.int64)


def tdm_apply(x_in, x_out, y, bank, plan, max_overlap_per_frame):
    """the two launches of one mixing: x_in -> x_out [n, C, N] (x_out may be x_in), y [n, T, W] in place, plan a host int32 [n, K, 4] array
    -> valid [n, K, max(1, longest st)] (device): the validity vector of every insertion"""
    import torch
    from . import _lib
    lib = _lib.load()
    n, Cc, N = x_in.shape
    T, W = int(y.shape[1]), int(y.shape[2])
    K = int(plan.shape[1])
    ld = max(1, int(plan[..., 1].max())) if plan.size else 1
    valid = torch.empty((n, K, ld), dtype=torch.float32, device=y.device)
    d_plan = torch.as_tensor(plan).to(y.device)
    st = C.c_void_p(torch.cuda.current_stream(y.device).cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = lib.seld_aug_tdm_labels(p(y), n, T, W, p(bank.bank_y), p(bank.d_row0), p(bank.d_rows), int(bank.rows.size), p(d_plan), K,
                                 int(max_overlap_per_frame), p(valid), ld, st)
    if rc:
        raise _lib.SeldError(rc, 'seld_aug_tdm_labels refused its arguments')
    rc = lib.seld_aug_tdm_mix(p(x_in), p(x_out), n, Cc, int(N), T, bank.spf, p(bank.bank_x), p(bank.d_s0), int(bank.rows.size), p(d_plan), K,
                              p(valid), ld, st)
    if rc:
        raise _lib.SeldError(rc, 'seld_aug_tdm_mix refused its arguments')
    return valid


def TDM_aug(x, y, tdm_x, tdm_y=None, sr=24000, label_resolution=0.1, max_overlap_num=5, max_overlap_per_frame=2, min_overlap_sec=1,
            max_overlap_sec=5, rng=None, draws=None, out=None, return_valid=False):
    """reference data_loader.TDM_aug (data_loader.py:188-234) on the device -> (x, y) [, valid].

    x: float32 device tensor [n, C, N] (mixed in place, or into `out`) or a list of n device tensors [C, N] (stacked: the result is one
    new tensor); y: float32 device tensor [n, T, 4*nc], updated in place.  The bank: the two lists of get_TDMset, or a TdmBank (tdm_y is
    then not needed) that packed them on the device once.  `draws`: a plan int [n, K, 4] = (cls, st, offset, td_offset) instead of rng's
    (checked on the host: ValueError).  Host tensors are refused: there is no CPU path."""
    import torch
    if isinstance(tdm_x, TdmBank):
        bank = tdm_x
    elif tdm_y is None or len(tdm_x) != len(tdm_y) or len(tdm_y) == 0:
        raise ValueError('TDM_aug: the bank is a TdmBank, or one waveform and one label track per class')
    else:
        bank = None
    rows = _tdm_bank_rows(tdm_x, tdm_y)
    xs = list(x) if isinstance(x, (list, tuple)) else None
    if not all(isinstance(t, torch.Tensor) for t in (xs if xs is not None else [x]) + [y]):
        raise ValueError('TDM_aug: x and y must be float32 CUDA tensors (the mixing runs on the device)')
    n = len(xs) if xs is not None else int(x.shape[0])
    if y.dim() != 3 or y.shape[0] != n or y.shape[2] % 4:
        raise ValueError(f'TDM_aug: y must be [{n}, T, 4 * n_classes], not {tuple(y.shape)}')
    T = int(y.shape[1])
    spf = int(sr * label_resolution)
    if draws is not None:
        plan = check_tdm_draws(draws, n, T, rows)
    else:
        plan = draw_tdm(rng or np.random.default_rng(), n, T, rows, int(max_overlap_num), tdm_frames(min_overlap_sec, label_resolution),
                        tdm_frames(max_overlap_sec, label_resolution))
    is_dev = lambda t: t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
    if not all(is_dev(t) for t in (xs if xs is not None else [x]) + [y]):
        raise ValueError('TDM_aug: x and y must be contiguous float32 CUDA tensors (the mixing runs on the device)')
    if xs is not None:
        x, out = torch.stack(xs), None
    if x.dim() != 3 or x.shape[2] < T * spf:
        raise ValueError(f'TDM_aug: x must be [{n}, C, N >= {T * spf}], not {tuple(x.shape)}')
    if out is None:
        out = x
    elif not is_dev(out) or out.shape != x.shape:
        raise ValueError('TDM_aug: out must be a contiguous float32 CUDA tensor of the shape of x')
    if bank is None:
        bank = TdmBank(tdm_x, tdm_y, sr, label_resolution, x.device)
    if bank.spf != spf or bank.W != y.shape[2] or bank.C != x.shape[1]:
        raise ValueError('TDM_aug: the bank was packed for another frame length, label width or channel count')
    valid = tdm_apply(x, out, y, bank, plan, max_overlap_per_frame)
    return (out, y, valid) if return_valid else (out, y)
