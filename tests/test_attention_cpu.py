"""The attention operators (include/seld_hip.h: seld_attn_*, seld_ln_*; seld_amd/csrc/attention.hip) and the transformer encoder block
(seld_amd/modules.py) as far as they can be checked without a GPU: the fp64 restatement tests/transformer_oracle.py pinned against torch's
own operators, the refusals of every new entry point (the pattern of tests/test_module_ops_cpu.py: a call that got as far as a launch
returns SELD_ERR_HIP here, so the return code shows that the refusal came first), the scratch sizes, and the configuration errors."""
import ctypes as C

import numpy as np
import pytest
import torch

import transformer_oracle as T
from helpers import rel_err
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


# ---------------------------------------------------------------- the stress inputs of tests/test_attention_gpu.py: what plain fp32 gives on them
FP32_CAP = 5e-5      # half the parity bar: a device miss of 1e-4 on these inputs is then the kernel's error, not the format's


def _attention_all(q, k, v, do, scale, dtype):
    tq, tk, tv = (torch.tensor(a, dtype=dtype, requires_grad=True) for a in (q, k, v))
    o, lse = T.attention(tq, tk, tv, scale)
    g = torch.autograd.grad((o * torch.tensor(do, dtype=dtype)).sum(), (tq, tk, tv))
    return [t.detach().double().numpy() for t in (o, lse) + g]


@pytest.mark.parametrize("kind,span,B,S,H,d", T.STRESS_CASES, ids=lambda v: str(v))
def test_stress_inputs_are_within_reach_of_fp32(kind, span, B, S, H, d):
    """every generator and shape the device runs: torch's fp32 on the CPU, forward and autograd backward, is within 5e-5 of the fp64 oracle
    under the project's metric; the inputs do what their names say; no gradient vanishes"""
    q, k, v, do, scale = T.stress_qkv(kind, span, B, S, H, d)
    for a in (q, k, v, do):
        assert a.dtype == np.float64 and np.array_equal(a, a.astype(np.float32).astype(np.float64))
    q2, k2, _, _, _ = T.stress_qkv(kind, span, B, S, H, d)
    assert np.array_equal(q, q2) and np.array_equal(k, k2)      # deterministic
    ref = _attention_all(q, k, v, do, scale, torch.float64)
    got = _attention_all(q, k, v, do, scale, torch.float32)
    for name, g, r in zip(("O", "lse", "dQ", "dK", "dV"), got, ref):
        e = rel_err(g, r)
        print(f"[fp32 cpu] {kind} span={span} d={d} {name}: {e:.3e} (|ref|max={np.abs(r).max():.3e})")
        assert e <= FP32_CAP, (name, e)
    assert min(np.abs(r).max() for r in ref[2:]) > 1e-2
    logits = np.einsum("bnhd,bmhd->bhnm", q, k) * scale
    pmax = np.exp(logits - ref[1][..., None]).max(-1)
    if kind == "gain":
        assert np.abs(logits).max() > 30 and pmax.mean() > 0.5
    else:
        first, last = logits[..., 0].mean(), logits[..., -1].mean()
        assert abs(abs(last - first) - span) < 1.0 and (last > first) == (kind == "ramp_up")
        if span >= 100 and kind != "shifted":
            assert logits.max() > 89      # past the range of fp32 exp: a softmax without the maximum subtraction overflows
        if kind == "shifted":
            assert logits.max() < -90      # ... and here it sums zeros


def _wave_sum(a):
    """[rows, 64] float32 -> [rows]: the xor-shuffle tree of a 64-lane wave, in fp32"""
    n = 64
    while n > 1:
        n //= 2
        a = a[:, :n] + a[:, n:2 * n]
    return a[:, 0]


def _lane_sums(a):
    """[rows, C] float32 -> [rows, 64]: lane l adds columns l, l + 64, ... in order, in fp32"""
    rows, Cc = a.shape
    pad = np.zeros((rows, -(-Cc // 64) * 64), np.float32)
    pad[:, :Cc] = a
    acc = np.zeros((rows, 64), np.float32)
    for j in range(pad.shape[1] // 64):
        acc = acc + pad[:, 64 * j:64 * j + 64]
    return acc


def _layer_norm_fp32(x, r, gamma, beta, one_pass):
    """LayerNorm of x + r in fp32 arithmetic throughout, one wave per row (lane-strided sums, then a tree): mean, then either the centred
    second moment (two passes) or E[z^2] - mean^2 (one pass)"""
    f = np.float32
    z = x.astype(f) + r.astype(f)
    Cc = f(z.shape[1])
    mean = _wave_sum(_lane_sums(z)) / Cc
    if one_pass:
        var = _wave_sum(_lane_sums(z * z)) / Cc - mean * mean
    else:
        t = z - mean[:, None]
        var = _wave_sum(_lane_sums(t * t)) / Cc
    rstd = f(1) / np.sqrt(var + f(T.LN_EPS))
    xhat = (z - mean[:, None]) * rstd[:, None]
    assert xhat.dtype == f
    return xhat * gamma.astype(f) + beta.astype(f), xhat, rstd


@pytest.mark.parametrize("mean,std,rows,Cc", T.LN_OFFSET_CASES)
def test_offset_rows_tell_a_two_pass_variance_from_a_one_pass_one(mean, std, rows, Cc):
    """on transformer_oracle.offset_rows a two-pass fp32 LayerNorm is within 5e-5 of the fp64 oracle and a one-pass fp32 variance misses the
    1e-4 bar: the device test on the same arrays has teeth"""
    x, r, dy, gamma, beta = T.offset_rows(mean, std, rows, Cc)
    for a in (x, r, dy, gamma, beta):
        assert np.array_equal(a, a.astype(np.float32).astype(np.float64))
    z = torch.tensor(x + r)
    assert float(z[1].std()) == 0.0 and float(z[2].std()) == 0.0 and float(torch.tensor(x)[1].std()) > 0.1
    assert np.array_equal((x.astype(np.float32) + r.astype(np.float32))[1:3], np.full((2, Cc), mean, np.float32))
    assert np.abs(np.log10(np.abs(gamma))).max() > 1.2 and beta.mean() > 49
    y_ref = T.layer_norm(z, torch.tensor(gamma), torch.tensor(beta)).numpy()
    zc = (z - z.mean(-1, keepdim=True)).numpy()
    rstd_ref = 1.0 / np.sqrt((zc ** 2).mean(-1) + T.LN_EPS)
    xhat_ref = zc * rstd_ref[:, None]
    two = [rel_err(g, f) for g, f in zip(_layer_norm_fp32(x, r, gamma, beta, False), (y_ref, xhat_ref, rstd_ref))]
    one = [rel_err(g, f) for g, f in zip(_layer_norm_fp32(x, r, gamma, beta, True), (y_ref, xhat_ref, rstd_ref))]
    print(f"[fp32 cpu] LayerNorm mean={mean} C={Cc}: two-pass y / xhat / rstd {two}, one-pass {one}")
    assert max(two) <= FP32_CAP
    assert min(one[:2]) > 1e-4      # y and xhat; rstd is measured against the constant rows' 1 / sqrt(eps) = 31.6, which hides the other rows' error


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


def _strides(op, ld):
    return {n: ld for n, kind, _ in OPS[op] if kind == "l"}


@pytest.mark.parametrize("op", ["seld_attn_fwd", "seld_attn_bwd"])
def test_refuses_heads_times_width_beyond_int(env, op):
    """H * d is formed in 64 bits: where it passes INT_MAX no int stride covers a row, whatever the 32-bit product wraps to (2^28 * 8 wraps
    to INT_MIN, 2^29 * 8 to 0, 2^28 * 24 to a positive value).  The pointers are never dereferenced: the refusal comes first."""
    for H, d in ((1 << 28, 8), (1 << 29, 8), (1 << 28, 24), (0x7fffffff, 64), (1 << 26, 32)):
        for ld in (16, 0x7fffffff):
            assert _call(env, op, H=H, d=d, **_strides(op, ld)) == INVALID, (H, d, ld)
    assert env[0].seld_attn_bwd_scratch(1, 3, 1 << 28, 8) == -1


@pytest.mark.parametrize("op", ["seld_attn_fwd", "seld_attn_bwd"])
def test_refuses_a_grid_beyond_int(env, op):
    """B * H * ceil(S / 64) workgroups beyond INT_MAX: UNSUPPORTED, also where a narrower product would wrap back into range (2^16 * 2^16 * 1 =
    2^32 -> 0; S = INT_MAX, whose S + 63 does not fit an int)"""
    for B, S, H in ((1 << 20, 8192, 32), (1 << 16, 3, 1 << 16), (64, 0x7fffffff, 1), (0x7fffffff, 0x7fffffff, 1 << 20), (1 << 24, 64 * 128 + 1, 1)):
        assert _call(env, op, B=B, S=S, H=H, d=8, **_strides(op, 8 * H)) == UNSUPPORTED, (B, S, H)
        assert env[0].seld_attn_bwd_scratch(B, S, H, 8) == -1
    # the largest grid that fits is not refused here: the scratch size says so without a launch
    assert env[0].seld_attn_bwd_scratch(1 << 20, 64 * 2047, 1, 8) == (1 << 20) * 64 * 2047


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
