"""Cases of the any-width attention (seld_attnw_* of seld_amd/csrc/attention.hip, modules' any_key_dim, ConvTemporalNet search=True) shared by
tests/test_attn_width_cpu.py and tests/test_attn_width_gpu.py: the kernel case lists, the inputs and their fp64 references
(transformer_oracle.attention, computed once per case and shared), the zero-padded operands of the padded-equivalence cases, the two block
cases and the model configuration."""
import functools
import math

import numpy as np
import torch

import conv_temporal_oracle as CT
import transformer_oracle as T

SEARCH_KEY_DIMS = [2, 3, 4, 6, 8, 12, 16, 24, 32, 48]      # nas_seldnet.search_space_1d_attention, both kinds
MAX_D = 64
B, H = 2, 3
PARITY_D = [1, 2, 3, 4, 6, 7, 9, 12, 15, 17, 31, 33, 47, 63]      # at S = 65: a second, nearly empty tile
EDGE_D, EDGE_S = [3, 12], [1, 63, 64, 65, 130]
PARITY_CASES = [(d, 65) for d in PARITY_D] + [(d, s) for d in EDGE_D for s in EDGE_S if s != 65]
PADDED_D, PADDED_S = [1, 3, 6, 12, 33, 63], [65, 130]
MULTIPLES = [8, 24, 64]
DROP = (0.3, 0x1234567890abcdef, 4098, 7)      # rate, seed, layer, step of the dropped cases
GUARD = 5                                        # odd: the fused buffer's row stride 3 H d + 5 is odd where H d is even
NAMES = ("O", "lse", "dQ", "dK", "dV")


def padded(d: int) -> int:
    return 8 * ((d + 7) // 8)


@functools.lru_cache(maxsize=None)
def inputs(S: int, d: int):
    """q, k, v, do: float32 numpy [B, S, H, d]"""
    rng = np.random.default_rng([S, d, 77])
    return tuple(T.f32(rng.standard_normal((B, S, H, d))) for _ in range(4))


@functools.lru_cache(maxsize=None)
def reference(S: int, d: int, dtype=torch.float64):
    """transformer_oracle.attention at scale 1 / sqrt(d) -> (o [R, H d], lse [B, H, S], dq, dk, dv [R, H d]) numpy"""
    q, k, v, do = inputs(S, d)
    tq, tk, tv = (torch.tensor(a, dtype=dtype, requires_grad=True) for a in (q, k, v))
    o, lse = T.attention(tq, tk, tv, 1.0 / math.sqrt(d))
    g = torch.autograd.grad((o * torch.tensor(do, dtype=dtype)).sum(), (tq, tk, tv))
    return [o.detach().numpy().reshape(B * S, H * d), lse.detach().numpy()] + [t.numpy().reshape(B * S, H * d) for t in g]


def zero_padded(a, d: int):
    """[B, S, H, d] -> [B, S, H, padded(d)] with zeros behind each head's d columns"""
    out = np.zeros(a.shape[:3] + (padded(d),), np.float32)
    out[..., :d] = a
    return out


def head_columns(a, S: int, dp: int, d: int):
    """[R, H dp] -> the first d columns of every head, [R, H d]"""
    return np.ascontiguousarray(a.reshape(B * S, H, dp)[:, :, :d]).reshape(B * S, H * d)


# ---------------------------------------------------------------- blocks through seld_amd.modules: (B, S, D, cfg)
TRANSFORMER_BLOCK = (2, 9, 10, {"n_head": 2, "key_dim": 3, "ff_multiplier": 2, "kernel_size": 3, "dropout_rate": 0, "activation": "relu"})
CONFORMER_BLOCK = (2, 9, 12, {"n_head": 3, "key_dim": 6, "kernel_size": 4, "multiplier": 2, "pos_encoding": None, "dropout_rate": 0})

# ---------------------------------------------------------------- the model: about gru_width_cases.CONFIG_A's size
CONFIG = {
    "n_classes": 3, "filters": 4, "first_kernel_size": 3, "first_pool_size": [2, 2],
    "BLOCK0": "transformer_encoder_stage",
    "BLOCK0_ARGS": {"depth": 1, "n_head": 2, "key_dim": 6, "ff_multiplier": 0.5, "kernel_size": 3, "dropout_rate": 0.0},
    "SED": "conformer_encoder_stage",
    "SED_ARGS": {"depth": 1, "key_dim": 12, "n_head": 2, "kernel_size": 4, "multiplier": 1, "pos_encoding": None, "dropout_rate": 0.0},
    "DOA": "bidirectional_GRU_stage", "DOA_ARGS": {"depth": 1, "units": 5},
}
INPUT = (3, 18, 8, 3)


def with_dropout(rate: float):
    cfg = {k: (dict(v) if isinstance(v, dict) else v) for k, v in CONFIG.items()}
    cfg["BLOCK0_ARGS"]["dropout_rate"] = cfg["SED_ARGS"]["dropout_rate"] = rate
    return cfg


@functools.lru_cache(maxsize=None)
def model_reference(dtype=torch.float64):
    """-> (w, st, x, ys, yd, ref): one train step and the inference of conv_temporal_oracle"""
    w, st = CT.random_weights(CONFIG, INPUT, seed=11)
    x, ys, yd = CT.synthetic_batch(CONFIG, INPUT, seed=23)
    ref = CT.train_step(CONFIG, INPUT, w, st, x, ys, yd, doa_loss="MSE", loss_weight=(1.0, 1000.0), lr=1e-3, step=1, dtype=dtype)
    ref["infer"] = CT.inference(CONFIG, INPUT, w, st, x, dtype=dtype)
    return w, st, x, ys, yd, ref
