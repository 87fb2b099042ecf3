"""seld_amd — MI355X-native SELDnet train/inference hot path (HIP kernels behind a C ABI).

Mirrors the interface of the reference IRIS-AUDIO/SELD for this path:
    models.seldnet(input_shape, model_config)      (reference models.py:18-32)
    models.seldnet_v1(input_shape, model_config)   (reference models.py:36-52)
    train.trainstep / train.teststep               (reference train.py:22-44)
    losses.MMSE, losses.MSE, losses.BinaryCrossentropy   (reference losses.py:4-13, train.py:311-320)
    nas_seldnet (conv_temporal_sampler, sample_constraint, train_and_eval, main) on models.conv_temporal(..., search=True): GRU stages of
        any width 1..256 on seld_rnn_gruw_fwd / _bwd (csrc/gru_w.hip)          (reference nas_seldnet.py, config_sampler.py:23-89)
PyTorch is used for device buffers, streams and torch.distributed only.
"""
from . import _lib  # noqa: F401
from . import losses, metrics, models, parallel, train, trainv2  # noqa: F401

__all__ = ["models", "losses", "train"]
