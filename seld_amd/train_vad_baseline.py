"""The voice-activity training recipe under the reference's names (train_vad_baseline.py): window batches from a packed corpus, an epoch loop
with early stopping on the validation AUC, and the whole-utterance evaluation — all on the device (seld_amd/vad.py, vad_dataloader.py,
vad_metrics.py).  There is no CPU or PyTorch fallback.

  prepare_dataset(pairs, window, batch_size, train=False, n_repeat=1, rng=None)   lines 26-35: an iterable; every pass over it is one epoch of
                                           VadDataset.batches (train: each pass shuffled), its window offsets drawn anew
  seq_to_windows, windows_to_seq           lines 76-106 (vad.py)
  train_and_eval(model_config, input_shape, trainset, valset, epochs, name, dropout=False, model=...)   lines 38-73: AdaBelief(1e-4), binary
                                           cross-entropy, validation AUC of the prediction monitored (mode max), patience 16, the best weights
                                           saved to {name}.npz and reloaded at the end -> (model, history).  model: "vad_architecture" — the
                                           model the reference trains — or "spectro_temporal_attention_based_VAD" (the default).
                                           `dropout` belongs to the default model alone (False: its dropout_rate must be 0); a
                                           vad_architecture's Dropout layers always draw, from the library's generator, at the rate its
                                           configuration gives, so dropout=True with it changes nothing and is accepted
  evaluate_pairs(model, pairs, window, batch_size)   lines 204-227: predict_sequence per utterance into one VADMetrics

An epoch enqueues every training and validation step — the window positions of each pass go up from pinned memory without a host wait
(VadDataset.batches) — and then reads the validation counters: the one point of an epoch where the host waits for the device.  The summed loss is
read right behind it from a stream that has already drained, and a new best adds the weight copy of its checkpoint.

Deviations: input_shape is [B, Wn, F, C] with the batch in front, as both models take it; the default model is
models.spectro_temporal_attention_based_VAD (the loss is the sum of its three outputs' cross-entropies, models_test.py:59-60), and
model="vad_architecture" trains the reference's models.vad_architecture on its one output (its label must have the prediction's shape:
[B, Wn] for last_unit = Wn behind flatten, or last_unit = 1 without it); the `res_*` stages of the reference's __main__ configuration are
not in its snapshot and not built; the checkpoint is an .npz, not an .h5; the reference's complexity report
(model_complexity.vad_architecture_complexity) is out of scope (VadArchNet.complexity() is our own count), so the second return value is the
history {loss, val_auc, val_precision, val_recall, val_f1, val_binary_accuracy}, one entry per epoch run."""
from __future__ import annotations

import numpy as np
import torch

from .trainv2 import AdaBelief
from .vad import SpectroTemporalVAD, model_out, predict_sequence, preprocess_window, seq_to_windows, windows_to_seq  # noqa: F401  (re-exported)
from .vad_dataloader import VadDataset, get_vad_dataset_from_pairs
from .vad_metrics import VADMetrics

PATIENCE = 16             # EarlyStopping(monitor='val_auc', patience=16, mode='max')
LEARNING_RATE = 1e-4      # AdaBelief(0.0001)


class _Epochs:
    """what prepare_dataset returns: iterating it once is one epoch"""

    def __init__(self, dataset: VadDataset, batch_size, train, n_repeat, rng):
        self.dataset, self.batch_size, self.train, self.n_repeat = dataset, int(batch_size), bool(train), int(n_repeat)
        self.rng = rng or np.random.default_rng()

    def __iter__(self):
        return self.dataset.batches(self.batch_size, self.n_repeat, shuffle=self.train, rng=self.rng)


def prepare_dataset(pairs, window, batch_size, train=False, n_repeat=1, rng=None):
    """pairs: a list of (features [frames, F, C], labels [frames]), or a VadDataset built with a window"""
    dataset = pairs if isinstance(pairs, VadDataset) else get_vad_dataset_from_pairs(pairs, window)
    if dataset.window is None:
        raise ValueError("prepare_dataset: the dataset holds no window (use_window=False)")
    return _Epochs(dataset, batch_size, train, n_repeat, rng)


def _validate(model, valset, metrics: VADMetrics):
    metrics.reset_states()
    for x, y in valset:
        metrics.update_state(y, model_out(model, x))


def _vad_architecture(input_shape, model_config, dropout):
    from .modules import VadArchNet      # its Dropout layers always draw from the library's generator: `dropout` has nothing to accept
    return VadArchNet(input_shape, model_config)


MODELS = {"spectro_temporal_attention_based_VAD": lambda shape, cfg, dropout: SpectroTemporalVAD(shape, cfg, dropout=dropout),
          "vad_architecture": _vad_architecture}


def train_and_eval(model_config: dict, input_shape, trainset, valset, epochs=1, name="bdnn_baseline", dropout=False,
                   model="spectro_temporal_attention_based_VAD"):
    """-> (model, history).  dropout: the default model only — SpectroTemporalVAD(dropout=...): False refuses a dropout_rate other than 0.
    model="vad_architecture" does not read it: simple_dense_block's Dropout draws whenever its dropout_rate is above 0 (set it to 0 to train
    without)."""
    if model not in MODELS:
        raise ValueError(f"model {model!r}: one of {tuple(MODELS)}")
    model = MODELS[model](input_shape, model_config, dropout)
    optimizer = AdaBelief(LEARNING_RATE)
    metrics = VADMetrics(device=model._dev.index)
    history = {k: [] for k in ("loss", "val_auc", "val_precision", "val_recall", "val_f1", "val_binary_accuracy")}
    path = f"{name}.npz"
    best, wait = -np.inf, 0
    for _ in range(int(epochs)):
        total, steps = torch.zeros((), dtype=torch.float32, device=model._dev), 0
        for x, y in trainset:
            total += model.train_step(x, y, optimizer)[1]
            steps += 1
        _validate(model, valset, metrics)
        res = metrics.result()                                   # the epoch's one synchronisation
        history["loss"].append(float(total) / max(steps, 1))
        for k, v in res.items():
            history[f"val_{k}"].append(v)
        if res["auc"] > best:                                    # ModelCheckpoint(save_best_only=True, mode='max')
            best, wait = res["auc"], 0
            model.save_weights(path)
        else:
            wait += 1
            if wait >= PATIENCE:
                break
    if np.isfinite(best):
        model.load_weights(path)
    return model, history


def evaluate_pairs(model, pairs, window, batch_size=None) -> dict:
    """{auc, precision, recall, f1, binary_accuracy} of the model's prediction (vad.model_out) over whole utterances: every utterance goes through predict_sequence
    (windows -> model -> windows_to_seq) and all of them into one VADMetrics"""
    window = preprocess_window(window)
    metrics = VADMetrics(device=model._dev.index)
    for x, y in pairs:
        y_hat = predict_sequence(model, x, window, batch_size)
        assert len(y) == len(y_hat), "lengths of labels and predictions are not equal"
        metrics.update_state(y, y_hat)
    return metrics.result()
