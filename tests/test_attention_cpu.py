"""The attention operators (include/seld_hip.h: seld_attn_*, seld_ln_*; seld_amd/csrc/attention.hip) and the transformer encoder block
(seld_amd/modules.py) as far as they can be checked without a GPU: the fp64 restatement tests/transformer_oracle.py pinned against torch's
own operators, the refusals of every new entry point (the pattern of tests/test_module_ops_cpu.py: a call that got as far as a launch
returns SELD_ERR_HIP here, so the return code shows that the refusal came first), the scratch sizes, and the configuration errors."""
import ctypes as C

import numpy as np
import pytest
import torch

import transformer_oracle as T
from seld_amd import _lib

INVALID, UNSUPPORTED, HIP = -1, -2, -3
BAD_D = (0, 4, 12, 65, 72)

# one valid call per operator: (argument name, kind, value).  kinds: p required pointer, o pointer that may be NULL, s size (refused at 0 and
# -1), l row stride (a size that must also be >= H * d), d the head width, v anything else.
OPS = {
    "seld_attn_fwd": [("Q", "p", 0), ("K", "p", 0), ("V", "p", 0), ("ldq", "l", 16), ("ldk", "l", 16), ("ldv", "l", 16), ("O", "p", 0), ("lse", "o", 0),
                      ("B", "s", 1), ("S", "s", 3), ("H", "s", 2), ("d", "d", 8), ("scale", "v", 0.5)],
    "seld_attn_bwd": [("Q", "p", 0), ("K", "p", 0), ("V", "p", 0), ("ldq", "l", 16), ("ldk", "l", 16), ("ldv", "l", 16), ("O", "p", 0), ("dO", "p", 0),
                      ("lse", "p", 0), ("dQ", "p", 0), ("dK", "p", 0), ("dV", "p", 0), ("lddq", "l", 16), ("lddk", "l", 16), ("lddv", "l", 16),
                      ("scratch", "p", 0), ("B", "s", 1), ("S", "s", 3), ("H", "s", 2), ("d", "d", 8), ("scale", "v", 0.5)],
    "seld_ln_fwd": [("x", "p", 0), ("r", "o", 0), ("gamma", "p", 0), ("beta", "p", 0), ("eps", "v", 1e-3), ("y", "p", 0), ("xhat", "o", 0),
                    ("rstd", "o", 0), ("rows", "s", 3), ("C", "s", 5)],
    "seld_ln_bwd": [("dy", "p", 0), ("xhat", "p", 0), ("rstd", "p", 0), ("gamma", "p", 0), ("dz", "p", 0), ("dgamma", "p", 0), ("dbeta", "p", 0),
                    ("scratch", "p", 0), ("rows", "s", 3), ("C", "s", 5)],
}
BUF_FLOATS = 1 << 12


@pytest.fixture(scope="module")
def env(seld_lib):
    gpu = torch.cuda.is_available()
    buf = torch.zeros(BUF_FLOATS, device="cuda") if gpu else None
    p = C.c_void_p(buf.data_ptr()) if gpu else C.c_void_p(1 << 20)     # no device: never dereferenced, a launch fails first
    yield seld_lib, p, gpu
    del buf


def _call(env, op, **over):
    lib, p, _ = env
    args = [over.get(name, p if kind in "po" else val) for name, kind, val in OPS[op]]
    return getattr(lib, op)(*args, None)      # the null stream


def _cases():
    for op, spec in OPS.items():
        for name, kind, _ in spec:
            if kind == "p":
                yield op, {name: None}
            elif kind in "sl":
                yield op, {name: 0}
                yield op, {name: -1}
            if kind == "l":
                yield op, {name: 15}      # H * d = 16


# ---------------------------------------------------------------- the oracle, pinned
def test_oracle_attention_is_scaled_dot_product_attention():
    g = torch.Generator().manual_seed(0)
    for B, S, H, d in ((2, 37, 3, 8), (1, 1, 2, 16), (2, 130, 4, 24)):
        q, k, v = (torch.randn(B, S, H, d, dtype=torch.float64, generator=g) for _ in range(3))
        scale = 0.37
        o, lse = T.attention(q, k, v, scale)
        ref = torch.nn.functional.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), scale=scale).transpose(1, 2)
        assert torch.allclose(o, ref, rtol=1e-12, atol=1e-12)
        logits = torch.einsum("bnhd,bmhd->bhnm", q, k) * scale
        assert torch.allclose(lse, torch.log(torch.exp(logits).sum(-1)), rtol=1e-12, atol=1e-12)


def test_oracle_layer_norm_is_layer_norm():
    g = torch.Generator().manual_seed(1)
    for rows, Cc in ((7, 8), (5, 4378), (3, 1)):
        x = torch.randn(rows, Cc, dtype=torch.float64, generator=g) * 3 + 1
        gamma, beta = torch.randn(Cc, dtype=torch.float64, generator=g), torch.randn(Cc, dtype=torch.float64, generator=g)
        ref = torch.nn.functional.layer_norm(x, (Cc,), gamma, beta, eps=T.LN_EPS)
        assert torch.allclose(T.layer_norm(x, gamma, beta), ref, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("D,H,dk,ffm,k", [(128, 4, 32, 2, 1), (96, 4, 24, 4, 3), (50, 3, 8, 1.5, 2)])
def test_block_parameter_count_is_the_closed_form(D, H, dk, ffm, k):
    cfg = {"n_head": H, "key_dim": dk, "ff_multiplier": ffm, "kernel_size": k, "dropout_rate": 0}
    specs = T.block_specs(D, cfg, "tf0")
    F = int(ffm * D)
    assert sum(int(np.prod(s)) for _, s in specs) == 4 * D * H * dk + 3 * H * dk + D + 2 * k * D * F + F + D + 4 * D
    assert [n.split(".", 1)[1] for n, _ in specs][:8] == ["mha.query.kernel", "mha.query.bias", "mha.key.kernel", "mha.key.bias", "mha.value.kernel",
                                                          "mha.value.bias", "mha.attention_output.kernel", "mha.attention_output.bias"]
    assert dict(specs)["tf0.mha.query.kernel"] == (D, H, dk) and dict(specs)["tf0.mha.attention_output.kernel"] == (H, dk, D)
    assert dict(specs)["tf0.ffn0.kernel"] == (k, D, F) and dict(specs)["tf0.ffn1.kernel"] == (k, F, D)
    # the restated block runs on these variables and the key bias has no gradient (softmax is shift-invariant along the keys)
    w = torch.tensor(T.random_block_weights(specs, 0), dtype=torch.float64, requires_grad=True)
    from oracle import seldnet_oracle as O
    x = torch.randn(2, 9, D, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    y = T.block_forward(x, O.unflatten(w, specs), "tf0", cfg)
    assert y.shape == x.shape
    (gw,) = torch.autograd.grad((y * torch.randn(y.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(3))).sum(), w)
    gd = O.unflatten(gw, specs)
    assert gd["tf0.mha.key.bias"].abs().max() <= 1e-12 * gw.abs().max() and gd["tf0.mha.query.bias"].abs().max() > 1e-6 * gw.abs().max()


# ---------------------------------------------------------------- refusals
@pytest.mark.parametrize("op", sorted(OPS))
def test_base_call_is_valid(env, op):
    assert _call(env, op) == (0 if env[2] else HIP)
    if env[2]:
        torch.cuda.synchronize()


@pytest.mark.parametrize("op,bad", list(_cases()), ids=lambda v: v if isinstance(v, str) else ",".join(f"{k}={v[k]}" for k in v))
def test_refuses_null_pointer_size_below_one_and_short_stride(env, op, bad):
    assert _call(env, op, **bad) == INVALID


@pytest.mark.parametrize("op", ["seld_attn_fwd", "seld_attn_bwd"])
def test_head_width_is_checked_first(env, op):
    """d is any multiple of 8 from 8 to 64; anything else is UNSUPPORTED even when another argument is bad as well (units in seld_m_gru_*)"""
    for d in BAD_D:
        assert _call(env, op, d=d, ldq=1024, ldk=1024, ldv=1024) == UNSUPPORTED
        assert _call(env, op, d=d, B=0) == UNSUPPORTED
        assert _call(env, op, d=d, Q=None) == UNSUPPORTED
        assert _call(env, op, d=d, ldq=-1) == UNSUPPORTED
    for d in range(8, 65, 8):
        assert _call(env, op, d=d, H=1, ldq=64, ldk=64, ldv=64, **({"lddq": 64, "lddk": 64, "lddv": 64} if op == "seld_attn_bwd" else {})) \
            == (0 if env[2] else HIP)
    if env[2]:
        torch.cuda.synchronize()


def test_optional_pointers_may_be_null(env):
    assert _call(env, "seld_attn_fwd", lse=None) == (0 if env[2] else HIP)
    assert _call(env, "seld_ln_fwd", r=None, xhat=None, rstd=None) == (0 if env[2] else HIP)
    if env[2]:
        torch.cuda.synchronize()


def test_scratch_sizes(seld_lib):
    lib = seld_lib
    for B, S, H, d in ((1, 1, 1, 8), (3, 61, 4, 24), (32, 600, 4, 48)):
        n = lib.seld_attn_bwd_scratch(B, S, H, d)
        assert n >= 1
        # linear in the rows: doubling S at most doubles it (plus a constant): no [S, S] buffer hides in the scratch
        c = 4096
        assert lib.seld_attn_bwd_scratch(B, 2 * S, H, d) <= 2 * n + c
        assert n <= 4 * B * H * S * (d + 2) + c          # and it is a few rows' worth, not a logits tensor
    for bad in (0, -1):
        assert lib.seld_attn_bwd_scratch(bad, 5, 2, 8) == -1
        assert lib.seld_attn_bwd_scratch(2, bad, 2, 8) == -1
        assert lib.seld_attn_bwd_scratch(2, 5, bad, 8) == -1
        assert lib.seld_ln_scratch(bad, 8) == -1
        assert lib.seld_ln_scratch(8, bad) == -1
    for d in BAD_D:
        assert lib.seld_attn_bwd_scratch(2, 5, 2, d) == -1
    for rows, Cc in ((1, 1), (3, 1), (60, 4378), (19200, 128)):
        n = lib.seld_ln_scratch(rows, Cc)
        assert 2 * Cc <= n <= 256 * 2 * Cc          # [first-stage workgroups <= 256][2][C]: bounded in the rows


# ---------------------------------------------------------------- configuration errors (no GPU: raised by the factories)
GOOD = {"depth": 2, "n_head": 4, "key_dim": 24, "ff_multiplier": 2, "kernel_size": 1, "dropout_rate": 0}


def test_factories_accept_a_good_configuration_without_a_device():
    from seld_amd import modules
    assert callable(modules.transformer_encoder_block(GOOD)) and callable(modules.transformer_encoder_stage(GOOD))
    assert callable(modules.transformer_encoder_block(dict(GOOD, activation="swish", dropout_rate=0.0)))
    assert set(modules.COMPOSED_SECOND) == {"bidirectional_GRU_block", "transformer_encoder_block", "transformer_encoder_stage"}


@pytest.mark.parametrize("bad", [{"dropout_rate": None}, {"dropout_rate": 0.1}, {"activation": "gelu"}, {"n_head": None}, {"key_dim": None},
                                 {"ff_multiplier": None}, {"kernel_size": None}, {"key_dim": 12}, {"key_dim": 72}],
                         ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items()))
def test_factories_refuse_bad_configurations(bad):
    """a missing (None here: the key is removed) or non-zero dropout_rate — the reference's default is 0.1 and there is no dropout kernel —
    an unknown activation, a missing mandatory key, a head width the kernels do not have"""
    from seld_amd import modules
    cfg = {k: v for k, v in dict(GOOD, **bad).items() if v is not None}
    with pytest.raises(ValueError) as e:
        modules.transformer_encoder_block(cfg)
    if "dropout_rate" in bad:
        assert "dropout" in str(e.value)
    with pytest.raises(ValueError):
        modules.transformer_encoder_stage(cfg)


def test_stage_needs_depth():
    from seld_amd import modules
    cfg = {k: v for k, v in GOOD.items() if k != "depth"}
    modules.transformer_encoder_block(cfg)
    with pytest.raises(ValueError):
        modules.transformer_encoder_stage(cfg)
