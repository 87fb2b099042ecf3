"""The evaluation of the voice-activity task (reference train_vad_baseline.py:49, 216-224): Keras AUC(), Precision(), Recall() and
binary_accuracy over whole utterances, plus the F1 the reference prints, from ONE set of device counters (seld_vad_score_update,
csrc/vad_feat.hip).  There is no CPU or PyTorch fallback for the counting.

  VADMetrics(num_thresholds=200)
    update_state(y, pred)   device tensors of any shape with equal element counts; asynchronous, no host synchronisation
    reset_states()
    result()                {auc, precision, recall, f1, binary_accuracy}: copies the 3 KB of counters (one synchronisation), then float64

Threshold table: Keras' AUC thresholds [-1e-7] + [(i + 1) / (T - 1) for i < T - 2] + [1 + 1e-7] merged with the 0.5 of Precision, Recall and
binary_accuracy, rounded to fp32 (Keras compares fp32 predictions with fp32 thresholds, strictly: pred > thr).  A prediction falls into bucket
k = the number of thresholds it exceeds; a NaN exceeds none.  Suffix sums over k give the true and false positives of every threshold.
  AUC (ROC, trapezoid)   sum_i (fpr[i] - fpr[i+1]) (tpr[i] + tpr[i+1]) / 2 over the T AUC thresholds; a ratio with a zero denominator is 0
  f1                     2 P R / (P + R + 1e-8)
Deviation: the reference accumulates its confusion counts in fp32 variables, which stop counting exactly at 2^24 elements per cell; these
counters are int64 and exact, and the rates are float64."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib

MAX_THRESHOLDS = 1024      # SCORE_MAX_NT (csrc/vad_feat.hip)


def auc_thresholds(num_thresholds: int = 200) -> np.ndarray:
    t = [-1e-7] + [(i + 1) / (num_thresholds - 1) for i in range(num_thresholds - 2)] + [1.0 + 1e-7]
    return np.asarray(t, np.float64).astype(np.float32)


def threshold_table(num_thresholds: int = 200) -> np.ndarray:
    """ascending fp32 [NT]: the AUC thresholds and 0.5, each value once"""
    if int(num_thresholds) != num_thresholds or not 2 <= num_thresholds < MAX_THRESHOLDS:
        raise ValueError(f"num_thresholds {num_thresholds!r}: an integer in 2 .. {MAX_THRESHOLDS - 1}")
    return np.unique(np.concatenate([auc_thresholds(int(num_thresholds)), np.float32([0.5])]))


def _div(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    out = np.zeros(np.broadcast(a, b).shape, np.float64)
    np.divide(a, b, out=out, where=b != 0)
    return out


def results_from_counts(counts: np.ndarray, num_thresholds: int = 200) -> dict:
    """counts int64 [NT + 1, 2] ([bucket, label bit]) -> the five figures, in float64"""
    thr = threshold_table(num_thresholds)
    c = np.asarray(counts, np.int64).reshape(len(thr) + 1, 2)
    above = np.cumsum(c[::-1], axis=0)[::-1][1:]      # [i]: elements whose prediction exceeds threshold i, per label bit
    fp, tp = above[:, 0].astype(np.float64), above[:, 1].astype(np.float64)
    n_neg, n_pos = float(c[:, 0].sum()), float(c[:, 1].sum())
    sel = np.searchsorted(thr, auc_thresholds(num_thresholds))
    tpr, fpr = _div(tp[sel], n_pos), _div(fp[sel], n_neg)
    auc = float(np.sum((fpr[:-1] - fpr[1:]) * (tpr[:-1] + tpr[1:]) / 2.0))
    h = int(np.searchsorted(thr, np.float32(0.5)))
    p, r = float(_div(tp[h], tp[h] + fp[h])), float(_div(tp[h], n_pos))
    acc = float(_div(tp[h] + n_neg - fp[h], n_pos + n_neg))
    return {"auc": auc, "precision": p, "recall": r, "f1": 2.0 * p * r / (p + r + 1e-8), "binary_accuracy": acc}


class VADMetrics:
    def __init__(self, num_thresholds: int = 200, device=None):
        self.num_thresholds = int(num_thresholds)
        table = threshold_table(num_thresholds)
        if not torch.cuda.is_available():
            raise RuntimeError("seld_amd needs a HIP device: there is no CPU fallback")
        self._dev = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
        self.lib = _lib.load()
        self.thresholds = torch.as_tensor(table).to(self._dev)
        self.counts = torch.zeros((len(table) + 1, 2), dtype=torch.int64, device=self._dev)

    def reset_states(self) -> None:
        self.counts.zero_()

    def update_state(self, y, pred) -> None:
        y = torch.as_tensor(y, dtype=torch.float32).to(self._dev).contiguous()
        pred = torch.as_tensor(pred, dtype=torch.float32).to(self._dev).contiguous()
        if y.numel() != pred.numel() or y.numel() < 1:
            raise ValueError(f"update_state: y {tuple(y.shape)} and pred {tuple(pred.shape)} must hold the same number (>= 1) of elements")
        st = C.c_void_p(torch.cuda.current_stream(self._dev).cuda_stream)
        _lib.check(self.lib.seld_vad_score_update(C.c_void_p(pred.data_ptr()), C.c_void_p(y.data_ptr()), y.numel(), C.c_void_p(self.thresholds.data_ptr()),
                                                  int(self.thresholds.numel()), C.c_void_p(self.counts.data_ptr()), st))

    def result(self) -> dict:
        return results_from_counts(self.counts.cpu().numpy(), self.num_thresholds)
