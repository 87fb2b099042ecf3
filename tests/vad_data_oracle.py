"""fp64 restatement of the voice-activity data path (seld_amd/csrc/vad_feat.hip, seld_amd/vad_dataloader.py, seld_amd/vad_metrics.py), in
this repository's own words: the mel matrix of tf.signal.linear_to_mel_weight_matrix, the unpadded stft front end with its per-file log and
min-max, frame labels, window batches and the threshold metrics of Keras AUC / Precision / Recall / binary_accuracy.  numpy and torch on the
CPU only.  The cases of tests/test_vad_data_cpu.py and tests/test_vad_data_gpu.py live here so that both judge the same inputs."""
from __future__ import annotations

import numpy as np
import torch

FLOOR = 1e-8
REF_WINDOW = [0, 9, 18, 19, 20, 29, 38]


# ---------------------------------------------------------------- mel matrix
def hz_to_mel(f):
    return 1127.0 * np.log1p(np.asarray(f, np.float64) / 700.0)


def mel_matrix(n_mels: int, n_bins: int, sample_rate: int, lower_hz: float = 0.0, upper_hz: float | None = None) -> np.ndarray:
    """[n_bins, n_mels] float64: triangles whose slopes are linear in mel, between n_mels + 2 edges equally spaced in mel; the DC row is zero"""
    upper_hz = sample_rate / 2.0 if upper_hz is None else float(upper_hz)
    bins = hz_to_mel(np.linspace(0.0, sample_rate / 2.0, n_bins))[:, None]
    edges = np.linspace(hz_to_mel(lower_hz), hz_to_mel(upper_hz), n_mels + 2)
    lo, mid, hi = edges[None, :-2], edges[None, 1:-1], edges[None, 2:]
    w = np.maximum(0.0, np.minimum((bins - lo) / (mid - lo), (hi - bins) / (hi - mid)))
    w[0] = 0.0
    return w


def n_frames(n_fft: int, n_samples: int) -> int:
    return 0 if n_samples < n_fft else 1 + (n_samples - n_fft) // (n_fft // 2)


# ---------------------------------------------------------------- front end
def magnitudes(wav, n_fft: int, dtype=torch.float64) -> torch.Tensor:
    """[frames, n_fft / 2 + 1]: periodic Hann, no centring, no padding, hop n_fft / 2"""
    x = torch.as_tensor(np.asarray(wav), dtype=dtype)
    win = torch.hann_window(n_fft, periodic=True, dtype=dtype)
    return torch.stft(x, n_fft, hop_length=n_fft // 2, win_length=n_fft, window=win, center=False, return_complex=True).abs().T


def front_end(wav, n_fft: int, n_mels: int, sample_rate: int, logmel: bool, normalize: bool, dtype=torch.float64) -> np.ndarray:
    """one file -> [frames, n_mels] in `dtype`'s arithmetic (float32: the plain restatement the fp32-room tests judge)"""
    mel = torch.as_tensor(mel_matrix(n_mels, n_fft // 2 + 1, sample_rate, 0.0, sample_rate // 2), dtype=dtype)
    s = magnitudes(wav, n_fft, dtype) @ mel
    with np.errstate(all="ignore"):
        if logmel:
            s = torch.log(torch.minimum(torch.clamp_min(s, FLOOR), s.max()))
        if normalize:
            s = (s - s.min()) / (s.max() - s.min())
    return s.numpy()


def pack(arrays):
    """arrays laid end to end -> (packed float32, starts int64 [n + 1])"""
    starts = np.concatenate([[0], np.cumsum([len(a) for a in arrays])]).astype(np.int64)
    return np.concatenate([np.asarray(a, np.float32) for a in arrays]), starts


def frame_starts(n_fft: int, lengths) -> np.ndarray:
    return np.concatenate([[0], np.cumsum([n_frames(n_fft, n) for n in lengths])]).astype(np.int64)


# ---------------------------------------------------------------- labels, windows
def frame_labels(labels, n_fft: int) -> np.ndarray:
    """round-half-even of the mean label of every frame"""
    lab = np.asarray(labels, np.float64)
    hop = n_fft // 2
    return np.array([np.rint(lab[j * hop:j * hop + n_fft].sum() / n_fft) for j in range(n_frames(n_fft, len(lab)))], np.float64)


def gather(feat, y, pos, window):
    idx = np.clip(np.asarray(pos, np.int64)[:, None] + np.asarray(window, np.int64)[None, :], 0, len(feat) - 1)
    return np.asarray(feat)[idx], np.asarray(y)[idx]


# ---------------------------------------------------------------- metrics
def thresholds(num: int = 200) -> np.ndarray:
    """the AUC thresholds of Keras merged with 0.5 (Precision, Recall, binary_accuracy), ascending, as fp32"""
    t = [-1e-7] + [(i + 1) / (num - 1) for i in range(num - 2)] + [1.0 + 1e-7]
    return np.unique(np.asarray(t + [0.5], np.float64).astype(np.float32))


def auc_thresholds(num: int = 200) -> np.ndarray:
    return np.asarray([-1e-7] + [(i + 1) / (num - 1) for i in range(num - 2)] + [1.0 + 1e-7], np.float64).astype(np.float32)


def bucket_counts(pred, y, thr) -> np.ndarray:
    """int64 [NT + 1, 2]: [k, label bit] with k the number of thresholds the fp32 prediction exceeds — counted directly, one comparison each"""
    p = np.asarray(pred, np.float32).reshape(-1)
    bit = (np.asarray(y, np.float32).reshape(-1) != 0).astype(np.int64)
    with np.errstate(invalid="ignore"):
        k = (p[:, None] > np.asarray(thr, np.float32)[None, :]).sum(1)
    c = np.zeros((len(thr) + 1, 2), np.int64)
    np.add.at(c, (k, bit), 1)
    return c


def _ratio(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.where(b != 0, a / np.where(b != 0, b, 1.0), 0.0)


def metrics_from_counts(counts, thr, num: int = 200) -> dict:
    c = np.asarray(counts, np.int64)
    tail = np.cumsum(c[::-1], axis=0)[::-1]          # tail[k] = elements in buckets >= k
    fp, tp = tail[1:, 0].astype(np.float64), tail[1:, 1].astype(np.float64)      # threshold i is exceeded by buckets > i
    neg, posn = float(c[:, 0].sum()), float(c[:, 1].sum())
    thr = np.asarray(thr, np.float32)
    sel = np.searchsorted(thr, auc_thresholds(num))
    assert np.array_equal(thr[sel], auc_thresholds(num))
    tpr, fpr = _ratio(tp[sel], posn), _ratio(fp[sel], neg)
    auc = float(np.sum((fpr[:-1] - fpr[1:]) * (tpr[:-1] + tpr[1:]) / 2.0))
    h = int(np.searchsorted(thr, np.float32(0.5)))
    assert thr[h] == np.float32(0.5)
    precision, recall = float(_ratio(tp[h], tp[h] + fp[h])), float(_ratio(tp[h], posn))
    acc = float(_ratio(tp[h] + (neg - fp[h]), neg + posn))
    return {"auc": auc, "precision": precision, "recall": recall, "f1": 2 * precision * recall / (precision + recall + 1e-8), "binary_accuracy": acc}


def metrics(pred, y, num: int = 200) -> dict:
    thr = thresholds(num)
    return metrics_from_counts(bucket_counts(pred, y, thr), thr, num)


# ---------------------------------------------------------------- cases
SR = 16000
FILE_LENGTHS = (1024, 1535, 1536, 3661, 2048)        # 1, 1, 2, 6, 3 frames at n_fft 1024
FILE_GAINS = (1.0, 1e-3, 0.3, 1.0, 0.05)
# (n_fft, n_mels, lengths, gains): three files each, one of them a single frame
SIZE_CASES = {
    "512x128": (512, 128, (512, 1300, 2049), (1.0, 0.02, 0.4)),
    "2048x7": (2048, 7, (5000, 2048, 6144), (0.5, 1.0, 0.01)),
    "512x80": (512, 80, (1279, 512, 2304), (1.0, 0.1, 3.0)),
}
FLAG_PAIRS = ((0, 0), (1, 0), (0, 1), (1, 1))


def noisy_files(lengths, gains, seed: int = 0):
    """N(0, 0.1) noise plus a 440 Hz tone, each file at its own gain (float32 values, as a decoded wav holds)"""
    rng = np.random.default_rng(seed)
    out = []
    for n, g in zip(lengths, gains):
        t = np.arange(n) / SR
        out.append((g * (0.1 * rng.standard_normal(n) + 0.5 * np.sin(2 * np.pi * 440.0 * t))).astype(np.float32))
    return out


def tone_file(n: int = 4096):
    return (0.5 * np.sin(2 * np.pi * 440.0 * np.arange(n) / SR)).astype(np.float32)


def binary_labels(lengths, seed: int = 1):
    """speech / non-speech runs of a few hundred samples"""
    rng = np.random.default_rng(seed)
    out = []
    for n in lengths:
        lab = np.zeros(n, np.float32)
        i, v = 0, int(rng.integers(0, 2))
        while i < n:
            run = int(rng.integers(100, 900))
            lab[i:i + run] = v
            i, v = i + run, 1 - v
        out.append(lab)
    return out


def score_inputs(n: int, labels: str, seed: int = 0, num: int = 200):
    """predictions that sit on every threshold itself, just above one, at 0, at 1 and on a NaN, the rest uniform; labels 'zeros' | 'ones' | 'mixed'"""
    rng = np.random.default_rng(seed)
    thr = thresholds(num)
    special = np.concatenate([thr, np.nextafter(thr, np.float32(np.inf)), np.float32([0.0, 1.0, np.nan])]).astype(np.float32)
    p = rng.random(n).astype(np.float32)
    if n >= len(special):
        p[rng.permutation(n)[:len(special)]] = special
    else:
        p[:] = special[rng.permutation(len(special))[:n]]
    y = {"zeros": np.zeros(n, np.float32), "ones": np.ones(n, np.float32), "mixed": (rng.random(n) < 0.4).astype(np.float32)}[labels]
    return p, y
