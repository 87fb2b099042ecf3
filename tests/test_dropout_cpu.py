"""CPU-side checks of the composed path's Dropout: what the factories accept and refuse, the C entry points' presence and
argument checks (nothing is enqueued), and the oracle's mask function (tests/dropout_oracle.py) against a hand-written Philox counter."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import dropout_oracle as DO
from conftest import ROOT
from oracle import seldnet_oracle as O

TRANSFORMER = {"depth": 2, "n_head": 4, "key_dim": 24, "ff_multiplier": 2, "kernel_size": 1}
CONFORMER = {"depth": 2, "n_head": 4, "key_dim": 24, "kernel_size": 24, "multiplier": 2}
ATTENTION = {"depth": 2, "key_dim": 16, "n_head": 4, "kernel_size": 3, "ff_kernel_size": 3, "ff_multiplier": 2, "ff_factor0": 1, "ff_factor1": 0.5,
             "abs_pos_encoding": True}
KINDS = {"transformer_encoder": TRANSFORMER, "conformer_encoder": CONFORMER, "attention": ATTENTION}


def _factories(kind):
    from seld_amd import modules
    return getattr(modules, kind + "_block"), getattr(modules, kind + "_stage")


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("rate", [0.1, None, 0, 0.5], ids=lambda r: f"rate={r}")
def test_factories_accept_a_dropout_rate(kind, rate):
    """0.1 — the reference's default (modules.py:386, 416, 529) — given or implied by an absent key (None here), 0 as before, and any rate below 1,
    for a caller that accepts the library's draws (dropout=True).  Without that the factories refuse what they refused before: the rate must be
    present and 0."""
    cfg = dict(KINDS[kind]) if rate is None else dict(KINDS[kind], dropout_rate=rate)
    for f in _factories(kind):
        assert callable(f(cfg, dropout=True))
        if rate == 0:
            assert callable(f(cfg))
        else:
            with pytest.raises(ValueError, match="dropout=True"):
                f(cfg)


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("rate", [1.0, -0.1, 1.5, float("nan")])
def test_factories_refuse_a_rate_outside_0_1(kind, rate):
    for f in _factories(kind):
        with pytest.raises(ValueError, match="dropout_rate"):
            f(dict(KINDS[kind], dropout_rate=rate), dropout=True)


@pytest.mark.parametrize("extra", [{"dropout_rate": 0.1}, {}, {"dropout_rate": 0.5, "pos_encoding": "basic"}], ids=str)
def test_relative_attention_block_refuses_dropout(extra):
    """seld_relattn_* has no dropped-probability form: abs_pos_encoding False takes dropout_rate 0 only (an absent key is the reference's 0.1)"""
    from seld_amd import modules
    cfg = dict({k: v for k, v in ATTENTION.items() if k != "abs_pos_encoding"}, **extra)
    for f in (modules.attention_block, modules.attention_stage):
        with pytest.raises(ValueError, match="abs_pos_encoding"):
            f(cfg, dropout=True)
        with pytest.raises(ValueError, match="dropout"):
            f(cfg)
        assert callable(f(dict(cfg, dropout_rate=0), dropout=True)) and callable(f(dict(cfg, dropout_rate=0)))
        assert callable(f(dict(cfg, dropout_rate=0.0, abs_pos_encoding=False), dropout=True))


def test_recurrent_blocks_and_heads_still_refuse_dropout():
    from seld_amd import modules
    with pytest.raises(ValueError, match="dropout"):
        modules.RNN_block({"units": 128, "dropout_rate": 0.3})
    with pytest.raises(TypeError):      # the recurrent factories have no draws to accept
        modules.RNN_block({"units": 128, "dropout_rate": 0.3}, dropout=True)
    with pytest.raises(ValueError, match="dropout"):
        modules.check_gru_config({"units": [128], "dropout_rate": 0.2})


def test_new_symbols_are_in_the_header_and_the_binding():
    from seld_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "seld_hip.h")).read(), flags=re.S)
    for name in ("seld_attn_drop_fwd", "seld_attn_drop_bwd", "seld_dropout"):
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES
    nf, nb = len(_lib.SIGNATURES["seld_attn_fwd"][1]), len(_lib.SIGNATURES["seld_attn_bwd"][1])
    assert len(_lib.SIGNATURES["seld_attn_drop_fwd"][1]) == nf + 4 and len(_lib.SIGNATURES["seld_attn_drop_bwd"][1]) == nb + 4
    assert _lib.SIGNATURES["seld_attn_drop_fwd"][1][:nf - 1] == _lib.SIGNATURES["seld_attn_fwd"][1][:nf - 1]      # the same arguments, then rate ...
    assert _lib.SIGNATURES["seld_attn_drop_bwd"][1][:nb - 1] == _lib.SIGNATURES["seld_attn_bwd"][1][:nb - 1]


def drop_entry_points_refuse_bad_arguments(lib, p):
    """the contract of seld_attn_* in the same order, + SELD_ERR_INVALID for a rate outside [0, 1), + SELD_ERR_UNSUPPORTED for a counter beyond 32
    bits; seld_dropout's.  `p`: any non-NULL pointer — every call returns before anything is enqueued.  Shared with tests/test_dropout_gpu.py."""
    INVALID, UNSUPPORTED = -1, -2
    seed = 0x5e1d5e1d5e1d5e1d
    fargs = (("Q", p), ("K", p), ("V", p), ("ldq", 16), ("ldk", 16), ("ldv", 16), ("O", p), ("lse", p), ("B", 1), ("S", 2), ("H", 2), ("d", 8),
             ("scale", 1.0), ("rate", 0.1), ("seed", seed), ("layer", 4096), ("step", 0), ("stream", None))
    bargs = (("Q", p), ("K", p), ("V", p), ("ldq", 16), ("ldk", 16), ("ldv", 16), ("O", p), ("dO", p), ("lse", p), ("dQ", p), ("dK", p), ("dV", p),
             ("lddq", 16), ("lddk", 16), ("lddv", 16), ("scratch", p), ("B", 1), ("S", 2), ("H", 2), ("d", 8), ("scale", 1.0), ("rate", 0.1),
             ("seed", seed), ("layer", 4096), ("step", 0), ("stream", None))
    fwd = lambda **kw: lib.seld_attn_drop_fwd(*[kw.get(n, d) for n, d in fargs])
    bwd = lambda **kw: lib.seld_attn_drop_bwd(*[kw.get(n, d) for n, d in bargs])
    for call, args in ((fwd, fargs), (bwd, bargs)):
        for d in (0, 4, 12, 72):
            assert call(d=d) == UNSUPPORTED
            assert call(d=d, Q=None, rate=2.0) == UNSUPPORTED          # the head width is judged first
        for name, dflt in args:
            if dflt is p and not (call is fwd and name == "lse"):
                assert call(**{name: None}) == INVALID, name
            elif name.startswith("ld"):
                assert call(**{name: 15}) == INVALID, name
        for name in ("B", "S", "H"):
            assert call(**{name: 0}) == INVALID
        for rate in (1.0, -0.1, 1.5, float("nan"), float("inf")):
            assert call(rate=rate) == INVALID, rate
            assert call(rate=rate, B=2 ** 20, S=2 ** 20) == INVALID      # ... before the grid
        assert call(B=2 ** 20, S=2 ** 20) == UNSUPPORTED                  # B * H * ceil(S / 64) beyond INT_MAX
        # the grid fits (65536 * 1025 workgroups) and (b H + h) S + n does not fit 32 bits: refused before anything is enqueued
        assert call(B=1024, S=65537, H=64, ldq=512, ldk=512, ldv=512, lddq=512, lddk=512, lddv=512) == UNSUPPORTED
    drop = lambda **kw: lib.seld_dropout(*[kw.get(n, d) for n, d in (("in", p), ("out", p), ("n", 5), ("rate", 0.1), ("alpha", 1.0),
                                                                         ("accumulate", 0), ("seed", seed), ("layer", 4096), ("step", 0),
                                                                         ("stream", None))])
    assert drop(**{"in": None}) == INVALID and drop(out=None) == INVALID
    assert drop(n=0) == INVALID and drop(n=-4) == INVALID
    for rate in (1.0, -0.1, float("nan")):
        assert drop(rate=rate) == INVALID


def test_entry_points_refuse_bad_arguments(seld_lib):
    buf = (C.c_float * 64)()
    drop_entry_points_refuse_bad_arguments(seld_lib, C.cast(buf, C.c_void_p))


# ---------------------------------------------------------------- the oracle's mask function
def _word(m4, layer, step, elem, seed, j):
    """word j of Philox4x32-10 at counter (m4, layer, step, elem) under the key (seed lo, seed hi)"""
    return int(O.philox4x32_10(np.uint64(m4), np.uint64(layer), np.uint64(step), np.uint64(elem), seed, seed >> 32)[j])


def test_attention_mask_follows_the_documented_counter():
    """M[b,h,n,m] at S = 5, H = 2, B = 2 for three elements, their counters written out by hand:
         first      (b, h, n, m) = (0, 0, 0, 0): counter (0, layer, step, 0), word 0
         wrap       (0, 1, 2, 3):                counter (0, layer, step, (0 * 2 + 1) * 5 + 2 = 7), word 3
         last       (1, 1, 4, 4):                counter (1, layer, step, (1 * 2 + 1) * 5 + 4 = 19), word 0"""
    B, S, H, layer, step, seed = 2, 5, 2, 4096 + 32 + 2, 9, DO.SEED
    named = {"first": ((0, 0, 0, 0), (0, 0, 0)), "wrap": ((0, 1, 2, 3), (0, 7, 3)), "last": ((1, 1, 4, 4), (1, 19, 0))}
    for rate in (0.1, 0.5):
        mask = DO.attention_mask(B, S, H, rate, seed, layer, step).numpy()
        assert mask.shape == (B, H, S, S)
        keep = 1.0 / (1.0 - float(np.float32(rate)))
        assert set(np.unique(mask)) <= {0.0, keep}
        for name, (idx, (m4, elem, j)) in named.items():
            u = (_word(m4, layer, step, elem, seed, j) >> 8) * 2.0 ** -24
            assert mask[idx] == (keep if u >= np.float32(rate) else 0.0), name
    # every element, the slow way
    rate = 0.5
    mask = DO.attention_mask(B, S, H, rate, seed, layer, step).numpy()
    for b in range(B):
        for h in range(H):
            for n in range(S):
                for m in range(S):
                    u = (_word(m >> 2, layer, step, (b * H + h) * S + n, seed, m & 3) >> 8) * 2.0 ** -24
                    assert (mask[b, h, n, m] != 0) == (u >= np.float32(rate))
    # a stream of its own per layer and per step
    assert not np.array_equal(mask, DO.attention_mask(B, S, H, rate, seed, layer + 1, step).numpy())
    assert not np.array_equal(mask, DO.attention_mask(B, S, H, rate, seed, layer, step + 1).numpy())


@pytest.mark.parametrize("rate", [0.1, 0.5])
def test_kept_fraction_of_the_draws(rate):
    """over n = 2^16 draws the kept fraction lies within four standard deviations of 1 - r: 4 sqrt(r (1 - r) / n)"""
    n = 2 ** 16
    bound = 4.0 * math.sqrt(rate * (1.0 - rate) / n)
    import torch
    m = O.dropout_mask((n,), rate, DO.SEED, 4096, 0, torch.float64).numpy()
    assert abs(float((m != 0).mean()) - (1.0 - rate)) <= bound
    am = DO.attention_mask(4, 64, 4, rate, DO.SEED, 4098, 0).numpy()      # 4 * 4 * 64 * 64 = 2^16 probabilities
    assert am.size == n and abs(float((am != 0).mean()) - (1.0 - rate)) <= bound


def test_stream_table():
    """layer = 4096 + 32 * block + site: clear of the fused path's 16 hd + j (< 64), 64 + i and 96 + 4 i + d (< 128), and of each other"""
    from seld_amd import modules
    assert modules.DROP_STREAM0 == DO.STREAM0 == 4096
    assert [len(v) for v in DO.STREAMS.values()] == [4, 7, 7]
    layers = [DO.Draws(0.1, i, 0).layer(s) for i in range(8) for s in range(7)]
    assert len(set(layers)) == len(layers) and min(layers) >= 4096
    for kind, sites in DO.STREAMS.items():
        assert sites.index("attention probabilities") == (0 if kind == "transformer" else 2)
        for s in sites:      # the docstring carries the table
            assert s.split()[-1] in modules._Drop.__doc__
