"""The conformer encoder block (seld_amd/modules.py, seld_amd/csrc/conformer.hip; reference modules.py:129-152, 410-508) as far as it can be
checked without a GPU: the fp64 restatement tests/conformer_oracle.py pinned against torch's own operators, the positional table against its
definition, the variable list and parameter count of the reference's own test configuration, the configuration refusals of the factories,
the argument refusals of the new entry points, and the condition under which the project's 1e-4 bar applies to the GPU cases unchanged: a
plain fp32 evaluation of each of them stays within 5e-5 of fp64."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conformer_oracle as K
import transformer_oracle as T
from helpers import rel_err

FP32_CAP = 5e-5


# ---------------------------------------------------------------- the oracle's pieces against torch's operators
@pytest.mark.parametrize("k", [1, 2, 3, 8, 31, 32])
def test_depthwise_conv_is_torch_conv1d_with_groups_and_tensorflow_same_padding(k):
    rng = np.random.default_rng(k)
    B, S, Cc = 2, 19, 5
    g, w, b = torch.tensor(rng.standard_normal((B, S, Cc))), torch.tensor(rng.standard_normal((k, 1, Cc))), torch.tensor(rng.standard_normal(Cc))
    pl = (k - 1) // 2
    ref = F.conv1d(F.pad(g.permute(0, 2, 1), (pl, k - 1 - pl)), w.permute(2, 1, 0), b, groups=Cc).permute(0, 2, 1)
    assert rel_err(K.depthwise_conv1d(g, w, b).numpy(), ref.numpy()) < 1e-13
    if k % 2 == 0:      # the mirrored split is a different function: the extra frame goes BEHIND
        wrong = F.conv1d(F.pad(g.permute(0, 2, 1), (k - 1 - pl, pl)), w.permute(2, 1, 0), b, groups=Cc).permute(0, 2, 1)
        assert rel_err(wrong.numpy(), ref.numpy()) > 1e-2


def test_glu_batch_norm_and_layer_norm_are_torchs():
    from oracle import seldnet_oracle as O
    rng = np.random.default_rng(0)
    u = torch.tensor(rng.standard_normal((2, 9, 12)))
    assert rel_err(K.glu(u).numpy(), F.glu(u, dim=-1).numpy()) < 1e-14
    z, gamma, beta = torch.tensor(rng.standard_normal((2, 9, 1, 6)) * 2 + 1), torch.tensor(rng.standard_normal(6)), torch.tensor(rng.standard_normal(6))
    mm, mv = torch.tensor(rng.standard_normal(6)), torch.tensor(1 + rng.random(6))
    y, nm, nv = O.batchnorm(z, gamma, beta, mm, mv, True)
    rm, rv = mm.clone(), mv.clone()
    ref = F.batch_norm(z.reshape(18, 6), rm, rv, gamma, beta, training=True, momentum=0.01, eps=1e-3)
    assert rel_err(y.reshape(18, 6).numpy(), ref.numpy()) < 1e-12 and rel_err(nm.numpy(), rm.numpy()) < 1e-12 and rel_err(nv.numpy(), rv.numpy()) < 1e-12
    y, _, _ = O.batchnorm(z, gamma, beta, mm, mv, False)
    assert rel_err(y.reshape(18, 6).numpy(), F.batch_norm(z.reshape(18, 6), mm, mv, gamma, beta, training=False, eps=1e-3).numpy()) < 1e-12
    x = torch.tensor(rng.standard_normal((4, 10)))
    assert rel_err(T.layer_norm(x, gamma.repeat(2)[:10], beta.repeat(2)[:10]).numpy(),
                   F.layer_norm(x, (10,), gamma.repeat(2)[:10], beta.repeat(2)[:10], eps=1e-3).numpy()) < 1e-12


def test_mha_ref_is_head_major_and_scales_the_query_after_its_bias():
    rng = np.random.default_rng(1)
    B, S, D, H, dk = 2, 7, 10, 3, 8
    cfg = {"n_head": H, "key_dim": dk}
    w = {f"m.{p}_kernel": torch.tensor(rng.standard_normal((H, D, dk))) for p in ("query", "key", "value")}
    w.update({"m.projection_kernel": torch.tensor(rng.standard_normal((H, dk, D))), "m.projection_bias": torch.tensor(rng.standard_normal(D))})
    w.update({f"m.{p}_bias": torch.tensor(rng.standard_normal((H, dk))) for p in "qkv"})
    x = torch.tensor(rng.standard_normal((B, S, D)))
    out = K.mha_ref(x, w, "m", cfg)
    acc = torch.zeros(B, S, D, dtype=torch.float64)
    for h in range(H):
        q = (x @ w["m.query_kernel"][h] + w["m.q_bias"][h]) / math.sqrt(dk)
        k = x @ w["m.key_kernel"][h] + w["m.k_bias"][h]
        v = x @ w["m.value_kernel"][h] + w["m.v_bias"][h]
        acc += torch.softmax(q @ k.transpose(1, 2), -1) @ v @ w["m.projection_kernel"][h]
    assert rel_err(out.numpy(), (acc + w["m.projection_bias"]).numpy()) < 1e-12
    # the same numbers read as [D, H, dk] are another function
    w2 = dict(w, **{f"m.{p}_kernel": w[f"m.{p}_kernel"].reshape(D, H, dk).permute(1, 0, 2) for p in ("query", "key", "value")})
    assert rel_err(K.mha_ref(x, w2, "m", cfg).numpy(), out.numpy()) > 1e-2


def test_positional_table_is_its_definition_and_the_products_own():
    from seld_amd import modules
    S, D = 600, 128
    t = K.pos_table(S, D)
    assert t.dtype == np.float32 and t.shape == (S, D)
    assert np.array_equal(t[0], np.tile(np.float32([1, 0]), D // 2))
    assert np.allclose(t[:, 1], np.sin(np.arange(S, dtype=np.float64)), atol=1e-7) and np.allclose(t[:, 0], np.cos(np.arange(S)), atol=1e-7)
    i = 5
    wi = np.float64(np.float32(10000.0 ** (-i / (D // 2))))
    assert np.allclose(t[:, 2 * i], np.cos(wi * np.arange(S)), atol=1e-7) and np.allclose(t[:, 2 * i + 1], np.sin(wi * np.arange(S)), atol=1e-7)
    assert np.array_equal(modules.basic_pos_encoding(S, D), t)      # the device adds the very table the oracle adds
    assert np.array_equal(modules.basic_pos_encoding(33, 50), K.pos_table(33, 50))
    # TensorFlow forms w * t in float32: the argument moves by at most half an ulp of 599
    arg32 = (np.float32(wi) * np.arange(S, dtype=np.float32)).astype(np.float64)
    assert np.abs(arg32 - wi * np.arange(S)).max() <= 2.0 ** -15


def test_oracle_sigmoid_has_torchs_values_and_the_true_derivative_where_it_saturates():
    """the values are torch.sigmoid's; the derivative at +-40 is exp(-40) / (1 + exp(-40))^2 = 4.25e-18 on both sides, where autograd through
    torch.sigmoid gives 0 at +40 in float64 (s (1 - s) on s rounded to 1) — the device is checked against the former"""
    b = torch.tensor([-40.0, -5.0, -0.3, 0.0, 0.3, 5.0, 40.0], dtype=torch.float64, requires_grad=True)
    assert rel_err(K.sigmoid(b).detach().numpy(), torch.sigmoid(b).detach().numpy()) < 1e-15
    (g,) = torch.autograd.grad(K.sigmoid(b).sum(), b)
    (naive,) = torch.autograd.grad(torch.sigmoid(b).sum(), b)
    e = math.exp(-40.0)
    true = e / (1.0 + e) ** 2
    assert abs(g[0].item() - true) <= 1e-12 * true and abs(g[-1].item() - true) <= 1e-12 * true
    assert naive[-1].item() == 0.0
    assert rel_err(g[1:-1].numpy(), naive[1:-1].numpy()) < 1e-14


# ---------------------------------------------------------------- variables
REF_TEST_CFG = {"depth": 2, "key_dim": 36, "n_head": 4, "kernel_size": 32, "multiplier": 4}      # the reference's stage test (defaults of modules.py:412-421)


def test_variable_list_and_parameter_count_of_the_reference_test_configuration():
    tr, nt = K.block_specs(64, REF_TEST_CFG, "cf0")
    count = lambda specs: sum(int(np.prod(s)) for _, s in specs)
    assert count(tr) == 118896 and count(nt) == 128
    # the closed forms of the reference's complexity accounting: LayerNormalization 2 D, Dense in * out + out, attention 4 H D dk + D + 3 H dk,
    # pointwise D * 2 D + 2 D, depthwise k D + D, BatchNormalization 2 D (+ 2 D moving), pointwise D D + D
    D, H, dk, k, m = 64, 4, 36, 32, 4
    closed = 5 * 2 * D + 2 * (D * m * D + m * D + m * D * D + D) + (4 * H * D * dk + D + 3 * H * dk) + (2 * D * D + 2 * D) + (k * D + D) + 2 * D + (D * D + D)
    assert closed == 118896
    order = [n.split(".", 1)[1] for n, _ in tr]
    assert order == ["ln0.gamma", "ln0.beta", "ffn0a.kernel", "ffn0a.bias", "ffn0b.kernel", "ffn0b.bias", "ln1.gamma", "ln1.beta",
                     "mha.query_kernel", "mha.key_kernel", "mha.value_kernel", "mha.projection_kernel", "mha.projection_bias", "mha.q_bias", "mha.k_bias",
                     "mha.v_bias", "ln2.gamma", "ln2.beta", "pw0.kernel", "pw0.bias", "dw.kernel", "dw.bias", "bn.gamma", "bn.beta", "pw1.kernel",
                     "pw1.bias", "ln3.gamma", "ln3.beta", "ffn1a.kernel", "ffn1a.bias", "ffn1b.kernel", "ffn1b.bias", "ln4.gamma", "ln4.beta"]
    shapes = dict((n.split(".", 1)[1], s) for n, s in tr)
    assert shapes["mha.query_kernel"] == (4, 64, 36) and shapes["mha.projection_kernel"] == (4, 36, 64) and shapes["mha.k_bias"] == (4, 36)
    assert shapes["pw0.kernel"] == (1, 64, 128) and shapes["dw.kernel"] == (32, 1, 64) and shapes["pw1.kernel"] == (1, 64, 64)
    assert shapes["ffn0a.kernel"] == (64, 256) and shapes["ffn1b.kernel"] == (256, 64)
    assert [n for n, _ in nt] == ["cf0.bn.moving_mean", "cf0.bn.moving_variance"]
    tr2, nt2 = K.stage_specs(64, REF_TEST_CFG, 2)
    assert count(tr2) == 2 * 118896 and count(nt2) == 256 and tr2[len(tr)][0] == "cf1.ln0.gamma"


def test_use_bias_false_removes_exactly_the_four_attention_biases():
    tr, _ = K.block_specs(64, REF_TEST_CFG, "b")
    tr0, _ = K.block_specs(64, dict(REF_TEST_CFG, use_bias=False), "b")
    gone = [n for n, _ in tr if n not in {m for m, _ in tr0}]
    assert gone == ["b.mha.projection_bias", "b.mha.q_bias", "b.mha.k_bias", "b.mha.v_bias"]
    assert [x for x in tr if x[0] not in gone] == tr0


# ---------------------------------------------------------------- configuration errors (no GPU: raised by the factories)
GOOD = {"depth": 2, "n_head": 4, "key_dim": 24, "kernel_size": 24, "multiplier": 2, "dropout_rate": 0}


def test_factories_accept_good_configurations_without_a_device():
    from seld_amd import modules
    assert callable(modules.conformer_encoder_block(GOOD)) and callable(modules.conformer_encoder_stage(GOOD))
    # what SS5.json passes: no positional encoding in the absolute mode means that none is added
    for extra in ({"pos_encoding": None}, {"pos_encoding": None, "pos_mode": "absolute"}, {"pos_encoding": "basic"}, {"activation": "relu"},
                  {"use_bias": False}, {"ffn_factor": 1.0}, {"kernel_regularizer": {"l1": 0.0, "l2": 1e-4}}, {"kernel_size": 64}, {"kernel_size": 1}):
        assert callable(modules.conformer_encoder_stage(dict(GOOD, **extra)))
    assert set(modules.CONFORMER_SECOND) == {"conformer_encoder_block", "conformer_encoder_stage"}
    assert not set(modules.CONFORMER_SECOND) & set(modules.COMPOSED_SECOND)


@pytest.mark.parametrize("bad", [{"dropout_rate": None}, {"dropout_rate": 0.1}, {"pos_mode": "relative"}, {"pos_encoding": "rff"},
                                 {"pos_encoding": "learned"}, {"key_dim": 36}, {"key_dim": None}, {"key_dim": 72}, {"n_head": 0}, {"kernel_size": 0},
                                 {"kernel_size": 65}, {"multiplier": 0}, {"activation": "gelu"}, {"kernel_regularizer": {"l3": 1.0}},
                                 {"kernel_regularizer": "l2"}],
                         ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items()))
def test_factories_refuse_what_has_no_kernel(bad):
    """a missing (None here: the key is removed, so the reference's default holds: dropout 0.1, key_dim 36) or non-zero dropout_rate,
    relative positions, the unreproducible random Fourier table, a head width the attention kernels do not have, sizes below one, a kernel
    longer than 64 frames, an unknown activation, a kernel_regularizer that is no l1 / l2 dict"""
    from seld_amd import modules
    cfg = {k: v for k, v in dict(GOOD, **bad).items() if v is not None}
    with pytest.raises(ValueError) as e:
        modules.conformer_encoder_block(cfg)
    if "dropout_rate" in bad:
        assert "dropout" in str(e.value)
    if "key_dim" in bad:
        assert "multiple of 8 from 8 to 64" in str(e.value)
    with pytest.raises(ValueError):
        modules.conformer_encoder_stage(cfg)


def test_stage_needs_a_depth_of_one_or_more():
    from seld_amd import modules
    cfg = {k: v for k, v in GOOD.items() if k != "depth"}
    modules.conformer_encoder_block(cfg)
    with pytest.raises(ValueError):
        modules.conformer_encoder_stage(cfg)
    with pytest.raises(ValueError):
        modules.conformer_encoder_stage(dict(GOOD, depth=0))


def test_basic_encoding_refuses_an_odd_width_before_any_device_is_touched():
    from seld_amd import modules
    with pytest.raises(ValueError) as e:
        modules.conformer_encoder_block(dict(GOOD, pos_encoding="basic"))((2, 10, 51))
    assert "odd" in str(e.value)
    with pytest.raises(ValueError):
        modules.conformer_encoder_block(GOOD)((2, 10, 17, 3))       # 'basic' is the default
    with pytest.raises(ValueError):
        modules.conformer_encoder_block(GOOD)((2, 10))


def test_conformer_stays_refused_as_first():
    from seld_amd import models
    with pytest.raises(ValueError):
        models._arch_from_config({"FIRST": "conformer_encoder_stage", "SECOND": "bidirectional_GRU_block", "SED": "simple_dense_block",
                                  "DOA": "simple_dense_block"}, 7, 64)


# ---------------------------------------------------------------- argument refusals of the entry points (no launch happens)
INVALID, UNSUPPORTED = -1, -2


def test_entry_points_refuse_bad_arguments(seld_lib):
    lib = seld_lib
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    fwd = lambda **kw: lib.seld_dwconv1d_fwd(*[kw.get(n, d) for n, d in (("u", p), ("ldu", 8), ("w", p), ("bias", p), ("y", p), ("B", 1), ("S", 2),
                                                                        ("C", 4), ("k", 3), ("glu", 1), ("stream", None))])
    bwd = lambda **kw: lib.seld_dwconv1d_bwd(*[kw.get(n, d) for n, d in (("u", p), ("ldu", 8), ("w", p), ("dy", p), ("du", p), ("lddu", 8), ("dw", p),
                                                                        ("dbias", p), ("scratch", p), ("B", 1), ("S", 2), ("C", 4), ("k", 3), ("glu", 1),
                                                                        ("stream", None))])
    for call, ptrs in ((fwd, ("u", "w", "bias", "y")), (bwd, ("u", "w", "dy", "du", "dw", "dbias", "scratch"))):
        for name in ptrs:
            assert call(**{name: None}) == INVALID, name
        for bad in ({"B": 0}, {"S": 0}, {"C": 0}, {"k": 0}, {"k": 65}, {"k": -1}, {"glu": 2}, {"glu": -1}, {"ldu": 7}, {"ldu": 4}, {"ldu": -8},
                    {"C": 1 << 30, "ldu": 0x7fffffff}, {"C": 0x7fffffff, "ldu": 0x7fffffff}):      # 2 C wraps in 32 bits
            assert call(**bad) == INVALID, bad
        assert call(glu=0, ldu=3) == INVALID
        wide = {"lddu": 128} if call is bwd else {}
        assert call(B=1 << 20, S=1 << 20, C=64, ldu=128, **wide) == UNSUPPORTED      # the grid
    assert bwd(lddu=7) == INVALID
    for bad in ((0, 5, 4, 3), (2, 0, 4, 3), (2, 5, 0, 3), (2, 5, 4, 0), (2, 5, 4, 65), (1 << 20, 1 << 20, 64, 3)):
        assert lib.seld_dwconv1d_bwd_scratch(*bad) == -1
    # bounded in the rows: [slots <= 512][k + 1][C]
    assert lib.seld_dwconv1d_bwd_scratch(1, 1, 1, 1) == 2
    assert lib.seld_dwconv1d_bwd_scratch(32, 600, 128, 32) == 320 * 33 * 128
    assert lib.seld_dwconv1d_bwd_scratch(4096, 600, 128, 32) == 512 * 33 * 128
    assert lib.seld_pos_add(None, p, 1, 2, 4, None) == INVALID and lib.seld_pos_add(p, p, 1, 0, 4, None) == INVALID
    assert lib.seld_head_permute(p, None, 2, 3, 8, 0, None) == INVALID and lib.seld_head_permute(p, p, 2, 3, 8, 2, None) == INVALID


# ---------------------------------------------------------------- the 1e-4 bar applies unchanged
@pytest.mark.parametrize("name", sorted(K.STAGE_CASES))
def test_plain_fp32_evaluation_of_every_gpu_case_is_within_5e_5_of_fp64(name):
    B, S, D, depth, cfg = K.STAGE_CASES[name]
    r64 = K.stage_reference(B, S, D, depth, cfg, seed=3, dtype=torch.float64)
    r32 = K.stage_reference(B, S, D, depth, cfg, seed=3, dtype=torch.float32)
    worst = max(rel_err(r32[key], r64[key]) for key in ("out_train", "out_eval", "new_state", "dx"))
    biggest = np.abs(r64["grad"]).max()
    off = 0
    for n, s in r64["specs"][0]:
        kk = int(np.prod(s))
        ref = r64["grad"][off:off + kk]
        if np.abs(ref).max() >= 1e-9 * biggest:
            worst = max(worst, rel_err(r32["grad"][off:off + kk], ref))
        off += kk
    print(f"[fp32 vs fp64] {name}: {worst:.3e}")
    assert worst <= FP32_CAP
    assert rel_err(r64["out_eval"], r64["out_train"]) > 1e-3      # training and inference are different functions here


@pytest.mark.parametrize("k,S,Cc,glu,span", [(32, 600, 128, True, 0.0), (8, 40, 65, True, 40.0), (31, 30, 7, False, 0.0), (64, 65, 64, True, 40.0)])
def test_plain_fp32_depthwise_is_within_5e_5_of_fp64(k, S, Cc, glu, span):
    u, w, b, dy = K.dwconv_inputs(2, S, Cc, k, glu, 0, span)
    r64, r32 = K.dwconv_reference(u, w, b, dy, glu), K.dwconv_reference(u, w, b, dy, glu, torch.float32)
    assert max(rel_err(a, r) for a, r in zip(r32, r64)) <= FP32_CAP
