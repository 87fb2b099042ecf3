"""The data path of the voice-activity task under the reference's names (vad_dataloader.py): wav -> unpadded stft magnitude -> mel -> log ->
per-file min-max on the device (seld_vad_feat_extract), sample labels -> frame labels (seld_vad_frame_labels), and one random window per
utterance per pass gathered into batches (seld_vad_gather); the kernels are csrc/vad_feat.hip.  There is no CPU or PyTorch fallback.

  get_mel_scale(n_fft, n_mels, sr)          tf.signal.linear_to_mel_weight_matrix(n_mels, n_fft // 2 + 1, sr, 0, sr // 2) as float32 numpy (host)
  preprocess_window                         vad.preprocess_window
  search_sub_dirs, extract_vad_fnames       the reference's file walk
  load_wav_and_extract_feat(name | array)   -> device [frames, n_mels, 1]; a path is read with the standard `wave` module: mono 16-bit PCM scaled
                                            by 1 / 32768 as tf.audio.decode_wav (anything else: ValueError)
  load_label(name | array)                  -> device [frames]
  extract_feat_label                        both, asserting equal lengths
  get_vad_dataset, get_vad_dataset_from_pairs -> VadDataset: a packed corpus (features [total_frames, F, C], labels [total_frames],
                                            frame_starts); a list of wavs is extracted in ONE seld_vad_feat_extract call
  VadDataset.batches(batch_size, n_repeat=1, shuffle=False, rng=None, draws=None)   yields device (x [b, Wn, F, C], y [b, Wn])

Semantics the kernels keep: no padding, no centring, hop n_fft / 2; the log's ceiling and the min-max run over one FILE;
a silent or constant file comes out all NaN, exactly as the reference's arithmetic gives — documented, not trapped.
Deviations: TensorFlow's generator cannot be reproduced, so the window offsets come from a numpy Generator (`rng`) or are given (`draws`, one
offset in [0, n_frames - max(window)) per utterance and pass, in corpus order), as seld_amd/transforms.py does; shuffle=True permutes each pass.
All positions of an epoch are drawn on the host and uploaded once, from pinned memory without a host wait.  get_vad_dataset refuses a wav whose
sample rate is not `sr` (the reference runs it through the mel table of `sr` silently).  Multi-channel wavs, resampling and hops other than
n_fft / 2 are not built.
ValueError, without a device, for a file shorter than n_fft, a file with n_frames <= max(window), and label and wav lengths that differ."""
from __future__ import annotations

import ctypes as C
import os
import wave
from typing import Sequence

import numpy as np
import torch

from . import _lib
from .vad import _table, preprocess_window  # noqa: F401  (re-exported)

N_FFT_SUPPORTED = (512, 1024, 2048)
MAX_MELS = 256      # SELD_VAD_MAX_MELS (include/seld_hip.h)


# ---------------------------------------------------------------- host helpers
def get_mel_scale(n_fft: int, n_mels: int, sr: int) -> np.ndarray:
    n_bins = int(n_fft) // 2 + 1
    w = np.empty((n_bins, int(n_mels)), np.float32)
    _lib.check(_lib.load().seld_vad_mel_matrix_host(int(n_mels), n_bins, int(sr), 0.0, float(int(sr) // 2), C.c_void_p(w.ctypes.data)))
    return w


def n_frames(n_fft: int, n_samples: int) -> int:
    return int(_lib.load().seld_vad_feat_frames(int(n_fft), int(n_samples)))


def search_sub_dirs(path, ext="wav"):
    """every *.ext file under `path`, at any depth (unsorted, as the directory walk yields them)"""
    suffix = "." + ext
    return [os.path.join(root, name) for root, _, names in os.walk(path) for name in names if name.endswith(suffix)]


def extract_vad_fnames(wav_folder, label_folder):
    """-> (the wavs under wav_folder, sorted; for each one the .npy of the same stem directly in label_folder)"""
    wavs = sorted(search_sub_dirs(wav_folder))
    return wavs, [os.path.join(label_folder, os.path.splitext(os.path.basename(w))[0] + ".npy") for w in wavs]


def read_wav(name):
    """-> (float32 [n_samples] in [-1, 1), sample rate): mono 16-bit PCM only"""
    with wave.open(os.fspath(name), "rb") as w:
        if w.getsampwidth() != 2 or w.getcomptype() != "NONE":
            raise ValueError(f"{name}: {8 * w.getsampwidth()}-bit {w.getcomptype()} samples: only 16-bit PCM is read (tf.audio.decode_wav)")
        if w.getnchannels() != 1:
            raise ValueError(f"{name}: {w.getnchannels()} channels: the VAD front end is mono")
        sr = w.getframerate()
        data = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")
    return data.astype(np.float32) / np.float32(32768.0), int(sr)


def _is_path(x) -> bool:
    return isinstance(x, (str, bytes, os.PathLike))


def _check_sizes(n_fft, n_mels):
    if int(n_fft) not in N_FFT_SUPPORTED:
        raise ValueError(f"n_fft {n_fft!r}: the front end's kernels take {N_FFT_SUPPORTED}")
    if not 1 <= int(n_mels) <= MAX_MELS:
        raise ValueError(f"n_mels {n_mels!r}: 1 .. {MAX_MELS}")


def _check_lengths(lengths: Sequence[int], n_fft: int, what="wav"):
    for i, n in enumerate(lengths):
        if n < n_fft:
            raise ValueError(f"{what} {i}: {n} samples hold no frame of n_fft {n_fft}")


def _check_window(frames: Sequence[int], window):
    width = int(np.max(window))
    for i, n in enumerate(frames):
        if n <= width:
            raise ValueError(f"utterance {i}: {n} frames hold no window of width {width} (n_frames must exceed max(window))")
    return width


def _device(device=None) -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("seld_amd needs a HIP device: there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device() if device is None else int(device))


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr())


# ---------------------------------------------------------------- the front end's handle
class _FrontEnd:
    """seld_vad_feat_create's handle for one (sr, n_fft, n_mels, device)"""
    _cache: dict = {}

    def __init__(self, sr, n_fft, n_mels, dev):
        self.lib = _lib.load()
        h = C.c_void_p()
        _lib.check(self.lib.seld_vad_feat_create(int(sr), int(n_fft), int(n_mels), dev.index, C.byref(h)))
        self.h = h

    @classmethod
    def get(cls, sr, n_fft, n_mels, dev):
        key = (int(sr), int(n_fft), int(n_mels), dev.index)
        if key not in cls._cache:
            cls._cache[key] = cls(*key[:3], dev)
        return cls._cache[key]      # ~30 KB of device tables, kept for the life of the process


def _tables(lengths, n_fft, dev):
    ss = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    fs = np.concatenate([[0], np.cumsum([n_frames(n_fft, n) for n in lengths])]).astype(np.int64)
    return ss, fs, torch.as_tensor(ss).to(dev), torch.as_tensor(fs).to(dev)


def extract_packed(wavs, n_fft=1024, n_mels=80, sr=16000, logmel=True, normalize=True, device=None):
    """a list of float32 arrays -> (features device [total_frames, n_mels], frame_starts numpy int64 [n + 1]) in one seld_vad_feat_extract call"""
    _check_sizes(n_fft, n_mels)
    wavs = [np.ascontiguousarray(np.asarray(w, np.float32).reshape(-1)) for w in wavs]
    if not wavs:
        raise ValueError("no utterance")
    lengths = [len(w) for w in wavs]
    _check_lengths(lengths, int(n_fft))
    dev = _device(device)
    fe = _FrontEnd.get(sr, n_fft, n_mels, dev)
    ss, fs, ss_d, fs_d = _tables(lengths, int(n_fft), dev)
    x = torch.as_tensor(np.concatenate(wavs)).to(dev)
    out = torch.empty((int(fs[-1]), int(n_mels)), dtype=torch.float32, device=dev)
    _lib.check(fe.lib.seld_vad_feat_extract(fe.h, _p(x), _p(ss_d), _p(fs_d), len(wavs), int(ss[-1]), int(fs[-1]), int(bool(logmel)), int(bool(normalize)),
                                            _p(out), _stream(dev)))
    return out, fs


def labels_packed(labels, n_fft=1024, device=None):
    """a list of sample-label arrays -> (frame labels device [total_frames], frame_starts)"""
    labels = [np.ascontiguousarray(np.asarray(a, np.float32).reshape(-1)) for a in labels]
    if not labels:
        raise ValueError("no utterance")
    if int(n_fft) < 2 or int(n_fft) % 2:
        raise ValueError(f"n_fft {n_fft!r}: an even frame length")
    lengths = [len(a) for a in labels]
    _check_lengths(lengths, int(n_fft), "label")
    dev = _device(device)
    ss, fs, ss_d, fs_d = _tables(lengths, int(n_fft), dev)
    x = torch.as_tensor(np.concatenate(labels)).to(dev)
    y = torch.empty(int(fs[-1]), dtype=torch.float32, device=dev)
    _lib.check(_lib.load().seld_vad_frame_labels(_p(x), _p(ss_d), _p(fs_d), len(labels), int(ss[-1]), int(fs[-1]), int(n_fft), _p(y), _stream(dev)))
    return y, fs


# ---------------------------------------------------------------- the reference's loaders
def _wav_of(name, sr):
    if _is_path(name):
        wav, file_sr = read_wav(name)
        return wav, file_sr
    return np.asarray(name, np.float32).reshape(-1), (16000 if sr is None else int(sr))


def load_wav_and_extract_feat(name, n_fft=1024, n_mels=80, mel_scale=None, logmel=True, normalize=True, sr=None, device=None, **kwargs):
    """vad_dataloader.py:77-98 -> device [frames, n_mels, 1].  `name`: a wav path or a float array of samples (then `sr`, default 16000).
    mel_scale: None, or exactly get_mel_scale(n_fft, n_mels, sr) (the filter table lives in the front end's handle: no other matrix is taken)"""
    _check_sizes(n_fft, n_mels)
    wav, file_sr = _wav_of(name, sr)
    sr = file_sr if sr is None else int(sr)
    if mel_scale is not None:
        m = np.asarray(mel_scale)
        if m.shape != (int(n_fft) // 2 + 1, int(n_mels)) or not np.array_equal(m.astype(np.float32), get_mel_scale(n_fft, n_mels, sr)):
            raise ValueError("mel_scale: only None or get_mel_scale(n_fft, n_mels, sr) — the kernels hold that matrix as a sparse table")
    out, _ = extract_packed([wav], n_fft, n_mels, sr, logmel, normalize, device)
    return out.unsqueeze(-1)


def _label_of(name):
    return np.load(os.fspath(name)) if _is_path(name) else np.asarray(name)


def load_label(name, n_fft=1024, device=None, **kwargs):
    """vad_dataloader.py:101-106 -> device [frames]: tf.round of every frame's mean label"""
    y, _ = labels_packed([_label_of(name)], n_fft, device)
    return y


def extract_feat_label(wav_fname, label_fname, **kwargs):
    """one utterance's (features [frames, n_mels, 1], frame labels [frames]); the two must hold the same number of frames"""
    pair = load_wav_and_extract_feat(wav_fname, **kwargs), load_label(label_fname, **kwargs)
    assert pair[0].shape[0] == pair[1].shape[0], f"{pair[0].shape[0]} feature frames against {pair[1].shape[0]} label frames"
    return pair


# ---------------------------------------------------------------- the packed corpus
class VadDataset:
    """features [total_frames, F, C] and labels [total_frames] on the device, utterance i owning rows frame_starts[i] .. frame_starts[i + 1];
    `window`: preprocess_window's offsets (None: use_window=False, no batches)"""

    def __init__(self, feats: torch.Tensor, labels: torch.Tensor, frame_starts, window=None):
        fs = np.asarray(frame_starts, np.int64).reshape(-1)
        if feats.dim() != 3 or labels.dim() != 1 or feats.shape[0] != labels.shape[0] or fs[0] != 0 or fs[-1] != feats.shape[0] or (np.diff(fs) < 1).any():
            raise ValueError(f"packed corpus: features {tuple(feats.shape)}, labels {tuple(labels.shape)}, frame_starts {fs.tolist()[:4]}..")
        self.feats, self.labels, self.frame_starts = feats.contiguous(), labels.contiguous(), fs
        self.window = None
        if window is not None:
            self.window, self._wp = _table(preprocess_window(window))
            self.width = _check_window(np.diff(fs), self.window)

    def __len__(self):
        return len(self.frame_starts) - 1

    def pairs(self):
        fs = self.frame_starts
        return [(self.feats[fs[i]:fs[i + 1]], self.labels[fs[i]:fs[i + 1]]) for i in range(len(self))]

    def draw(self, n_repeat=1, rng=None) -> np.ndarray:
        """int64 [n_repeat * n]: one offset in [0, n_frames - max(window)) per utterance and pass"""
        rng = rng or np.random.default_rng()
        room = np.tile(np.diff(self.frame_starts) - self.width, int(n_repeat))
        return rng.integers(0, room)

    def positions(self, n_repeat=1, shuffle=False, rng=None, draws=None) -> np.ndarray:
        """the absolute first rows of every window of an epoch, in the order the batches take them"""
        if self.window is None:
            raise ValueError("this dataset was built with use_window=False")
        n, n_repeat = len(self), int(n_repeat)
        if n_repeat < 1:
            raise ValueError("n_repeat >= 1")
        rng = rng or np.random.default_rng()
        room = np.tile(np.diff(self.frame_starts) - self.width, n_repeat)
        off = self.draw(n_repeat, rng) if draws is None else np.asarray(draws, np.int64).reshape(-1)
        if off.shape != room.shape or (off < 0).any() or (off >= room).any():
            raise ValueError(f"draws: {n_repeat * n} offsets, each in [0, n_frames - {self.width})")
        pos = np.tile(self.frame_starts[:-1], n_repeat) + off
        if shuffle:
            pos = np.concatenate([pos[r * n:(r + 1) * n][rng.permutation(n)] for r in range(n_repeat)])
        return pos.astype(np.int64)

    def batches(self, batch_size, n_repeat=1, shuffle=False, rng=None, draws=None):
        batch_size = int(batch_size)
        if batch_size < 1:
            raise ValueError("batch_size >= 1")
        # one upload per epoch, from pinned memory: the copy is enqueued on the stream and the host does not wait for it (`host` stays alive in
        # this generator's frame until the last batch is taken)
        host = torch.as_tensor(self.positions(n_repeat, shuffle, rng, draws)).pin_memory()
        pos = host.to(self.feats.device, non_blocking=True)
        lib, dev = _lib.load(), self.feats.device
        Wn, (F, Cc) = int(self.window.size), self.feats.shape[1:]
        for i in range(0, pos.numel(), batch_size):
            b = min(batch_size, pos.numel() - i)
            x = torch.empty((b, Wn, F, Cc), dtype=torch.float32, device=dev)
            y = torch.empty((b, Wn), dtype=torch.float32, device=dev)
            _lib.check(lib.seld_vad_gather(_p(self.feats), _p(self.labels), C.c_void_p(pos.data_ptr() + 8 * i), self._wp, Wn, b, int(F * Cc),
                                           int(self.feats.shape[0]), _p(x), _p(y), _stream(dev)))
            yield x, y


def get_vad_dataset(wav_fnames, label_fnames, window, n_fft=1024, n_mels=80, sr=16000, use_window=True, logmel=True, normalize=True, device=None,
                    **kwargs) -> VadDataset:
    """vad_dataloader.py:26-54: wav_fnames / label_fnames are paths or arrays.  Every refusal comes before the device is touched."""
    if len(wav_fnames) != len(label_fnames) or len(wav_fnames) < 1:
        raise ValueError(f"{len(wav_fnames)} wavs and {len(label_fnames)} labels")
    _check_sizes(n_fft, n_mels)
    wavs = []
    for i, w in enumerate(wav_fnames):
        x, file_sr = _wav_of(w, sr)
        if file_sr != int(sr):      # the reference would run such a file through the mel table of `sr` without a word; nothing here resamples
            raise ValueError(f"utterance {i}: recorded at {file_sr} Hz, the dataset is built for sr {sr}")
        wavs.append(x)
    labels = [np.asarray(_label_of(a), np.float32).reshape(-1) for a in label_fnames]
    for i, (w, a) in enumerate(zip(wavs, labels)):
        if len(w) != len(a):
            raise ValueError(f"utterance {i}: {len(w)} samples and {len(a)} labels")
    _check_lengths([len(w) for w in wavs], int(n_fft))
    if use_window:
        window = preprocess_window(window)
        _check_window([n_frames(n_fft, len(w)) for w in wavs], window)
    feats, fs = extract_packed(wavs, n_fft, n_mels, sr, logmel, normalize, device)
    y, _ = labels_packed(labels, n_fft, device)
    return VadDataset(feats.unsqueeze(-1), y, fs, window if use_window else None)


def get_vad_dataset_from_pairs(feat_label_pairs, window, device=None) -> VadDataset:
    """vad_dataloader.py:57-74: pairs of (features [frames, n_mels, n_chan], labels [frames]), arrays or tensors"""
    if len(feat_label_pairs) < 1:
        raise ValueError("no pair")
    window = preprocess_window(window)
    frames = []
    for i, (f, a) in enumerate(feat_label_pairs):
        if len(f.shape) != 3 or len(a.shape) != 1 or f.shape[0] != a.shape[0] or tuple(f.shape[1:]) != tuple(feat_label_pairs[0][0].shape[1:]):
            raise ValueError(f"pair {i}: features {tuple(f.shape)} and labels {tuple(a.shape)}: [frames, n_mels, n_chan] and [frames]")
        frames.append(int(f.shape[0]))
    _check_window(frames, window)
    dev = _device(device)
    to = lambda t: torch.as_tensor(t, dtype=torch.float32).to(dev)
    feats = torch.cat([to(f) for f, _ in feat_label_pairs], dim=0)
    labels = torch.cat([to(a) for _, a in feat_label_pairs], dim=0)
    return VadDataset(feats, labels, np.concatenate([[0], np.cumsum(frames)]), window)
