"""What can be held without a device about attention_block / attention_stage and relative-position attention (reference modules.py:155-180,
511-635, layers.py:332-392): the index identity seld_amd/csrc/relattn.hip runs on against the literal pad / reshape shift, the variable lists,
the factories' acceptances and refusals, the C entry points' argument checks, and that a plain fp32 evaluation of every GPU case of
tests/test_attention_block_gpu.py stays within 5e-5 of fp64 (so the 1e-4 bar applies there unchanged)."""
import ctypes as C

import numpy as np
import pytest
import torch

import attention_block_oracle as A
from helpers import rel_err

FP32_CAP = 5e-5
INVALID, UNSUPPORTED = -1, -2


# ---------------------------------------------------------------- the shift
@pytest.mark.parametrize("S", [1, 2, 3, 7, 64, 65])
def test_closed_form_index_identity_is_the_literal_shift(S):
    """shifted[i,j] = G[i, S-1-i+j] (j <= i), exactly 0 on j = i+1, G[i+1, j-i-2] (j >= i+2: the NEXT query row)"""
    G = torch.arange(1, 2 * 3 * S * S + 1, dtype=torch.float64).reshape(2, 3, S, S)      # every element distinct and non-zero
    lit = A.relative_shift(G)
    assert torch.equal(lit, A.shift_closed_form(G))
    for i in range(S - 1):
        assert float(lit[..., i, i + 1].abs().max()) == 0.0
    for i in range(S - 2):
        for j in range(i + 2, S):
            assert torch.equal(lit[..., i, j], G[..., i + 1, j - i - 2])
    # the band form of the kernels: Pext = the table and a zero row, index (S - 1 - i + j) mod (S + 1), the query row i + [j > i]
    ext = torch.cat([G, torch.zeros(2, 3, 1, S, dtype=G.dtype)], dim=2)      # a zero QUERY row S for the row i + 1 = S that no valid j reads
    ext = torch.cat([ext, torch.zeros(2, 3, S + 1, 1, dtype=G.dtype)], dim=3)
    for i in range(S):
        for j in range(S):
            assert torch.equal(lit[..., i, j], ext[..., i + int(j > i), (S - 1 - i + j) % (S + 1)])


@pytest.mark.parametrize("S", [1, 2, 3, 7, 65])
def test_use_once_map_is_autograds_gradient_of_the_literal_shift(S):
    """every G[i,m] is read by one logit at most, G[0, m <= S-2] by none: the backward of the shift is a re-indexing"""
    G = torch.randn(S, S, dtype=torch.float64, requires_grad=True)
    dS = torch.randn(S, S, dtype=torch.float64)
    (dG,) = torch.autograd.grad((A.relative_shift(G[None, None])[0, 0] * dS).sum(), G)
    m = A.use_once_map(S)
    mine = torch.zeros(S, S, dtype=torch.float64)
    for (i, mm), (ii, j) in m.items():
        mine[i, mm] = dS[ii, j]
    assert torch.equal(dG, mine)
    assert len(set(m.values())) == len(m) and len(m) == S * S - (S - 1)
    assert all((0, mm) not in m for mm in range(S - 1))


def test_rel_attention_without_positions_is_plain_attention_and_scales_the_sum():
    q, k, v, P, u, vb, do, scale = (torch.tensor(a) if isinstance(a, np.ndarray) else a for a in A.relattn_inputs(2, 9, 2, 8))
    o, lse = A.rel_attention(q, k, v, 0 * P, 0 * u, 0 * vb, scale)
    o2, lse2 = A.T.attention(q * scale, k, v, 1.0)
    assert rel_err(o.numpy(), o2.numpy()) < 1e-14 and rel_err(lse.numpy(), lse2.numpy()) < 1e-14
    o3, _ = A.rel_attention(q, k, v, P, u, vb, scale)
    assert rel_err(o3.numpy(), o.numpy()) > 1e-2


# ---------------------------------------------------------------- variables
count = lambda specs: sum(int(np.prod(s)) for _, s in specs)
conv1d_params = lambda k, c, f, groups=1: k * c * f // groups + f                                  # complexity.conv1d_complexity
norm_params = lambda c: 2 * c                                                                       # complexity.norm_complexity


def mha_params(c, H, dk, rel, bias):
    """complexity.multi_head_attention_complexity (value_dim = key_dim)"""
    return H * (c + bias) * 3 * dk + (H * dk * 2 + H * dk * c if rel else 0) + H * c * dk + c * bias


def test_variables_of_the_reference_test_attention_block():
    """modules_test.py:295-317: relative attention, GLU, kernel_size 0 (x = GLU(Conv1D(2D, 1)(x))), layer norms behind"""
    D = 64
    tr, nt = A.block_specs(D, A.REF_BLOCK, "at0")
    names = [n.split(".", 1)[1] for n, _ in tr]
    assert names == ["ff0a.kernel", "ff0a.bias", "ff0b.kernel", "ff0b.bias", "ln0.gamma", "ln0.beta", "mha.pos_kernel", "mha.pos_bias_u",
                     "mha.pos_bias_v", "mha.query_kernel", "mha.key_kernel", "mha.value_kernel", "mha.projection_kernel", "ln1.gamma", "ln1.beta",
                     "pw0.kernel", "pw0.bias", "ff1a.kernel", "ff1a.bias", "ff1b.kernel", "ff1b.bias", "ln3.gamma", "ln3.beta"]
    assert nt == []
    assert dict(tr)["at0.mha.pos_kernel"] == (4, 64, 16) and dict(tr)["at0.ff0a.kernel"] == (3, 64, 128) and dict(tr)["at0.pw0.kernel"] == (1, 64, 128)
    ff = conv1d_params(3, D, 2 * D) + conv1d_params(3, 2 * D, D) + norm_params(D)
    # attention_block_complexity for this configuration: FF, norm + attention, GLU conv, FF (no layer is dead here)
    assert count(tr) == ff + norm_params(D) + mha_params(D, 4, 16, True, 0) + conv1d_params(1, D, 2 * D) + ff


def test_variables_of_the_reference_test_attention_stage():
    """modules_test.py:129-152: MultiHeadAttention_, layer norms in front, a depthwise module without GLU, no first FF.  The FF module's own
    LayerNormalization is dead (its output is discarded): attention_block_complexity counts one norm there, the model has none."""
    D = 64
    tr, nt = A.stage_specs(D, A.REF_STAGE, 3)
    names = [n.split(".", 1)[1] for n, _ in tr if n.startswith("at1.")]
    assert names == ["ln1.gamma", "ln1.beta", "mha.query_kernel", "mha.key_kernel", "mha.value_kernel", "mha.projection_kernel", "ln2.gamma", "ln2.beta",
                     "dw.kernel", "dw.bias", "bn.gamma", "bn.beta", "pw1.kernel", "pw1.bias", "ff1a.kernel", "ff1a.bias", "ff1b.kernel", "ff1b.bias"]
    assert [n for n, _ in nt] == [f"at{i}.bn.moving_{m}" for i in range(3) for m in ("mean", "variance")]
    per_block = (norm_params(D) + mha_params(D, 4, 16, False, 0) + norm_params(D) + conv1d_params(3, D, D, groups=D) + norm_params(D)
                 + conv1d_params(1, D, D) + norm_params(D) + conv1d_params(3, D, 2 * D) + conv1d_params(3, 2 * D, D))      # complexity's count
    assert count(tr) == 3 * (per_block - norm_params(D))      # minus the dead FF LayerNormalization
    assert not any(".ln3." in n or ".ln0." in n for n, _ in tr)


def test_use_bias_adds_exactly_the_four_attention_biases_behind_the_projection_kernel():
    for cfg in (A.REF_BLOCK, A.REF_STAGE):
        tr0, _ = A.block_specs(64, cfg, "b")
        tr1, _ = A.block_specs(64, dict(cfg, use_bias=True), "b")
        extra = [n for n, _ in tr1 if (n, dict(tr1)[n]) not in tr0]
        assert extra == ["b.mha.projection_bias", "b.mha.q_bias", "b.mha.k_bias", "b.mha.v_bias"]
        i = [n for n, _ in tr1].index("b.mha.projection_kernel")
        assert [n for n, _ in tr1][i + 1:i + 5] == extra
        assert count(tr1) - count(tr0) == 64 + 3 * 4 * 16


def test_layer_norm_positions_with_glu_and_depthwise():
    """quirk 4: with layer_norm_in_front the GLU / depthwise part has ONE LayerNormalization — in front of the pointwise conv with use_glu, else
    in front of the depthwise conv; behind, one after the residual"""
    cfg = dict(A.REF_BLOCK, kernel_size=3)
    order = lambda c: [n.split(".")[1] for n, _ in A.block_specs(32, c, "b")[0] if n.endswith((".kernel", ".gamma")) and ".mha." not in n and ".ff" not in n]
    assert order(dict(cfg, layer_norm_in_front=True, use_glu=True)) == ["ln1", "ln2", "pw0", "dw", "bn", "pw1"]
    assert order(dict(cfg, layer_norm_in_front=True, use_glu=False)) == ["ln1", "ln2", "dw", "bn", "pw1"]
    assert order(dict(cfg, layer_norm_in_front=False, use_glu=True)) == ["ln0", "ln1", "pw0", "dw", "bn", "pw1", "ln2", "ln3"]
    assert order(dict(cfg, layer_norm_in_front=True, use_glu=True, kernel_size=0)) == ["ln1", "ln2", "pw0"]


# ---------------------------------------------------------------- factories
GOOD = dict(A.REF_BLOCK, depth=2)


def test_factories_accept_good_configurations_without_a_device():
    from seld_amd import modules
    assert modules.ATTENTION_SECOND == ("attention_block", "attention_stage")
    assert callable(modules.attention_block(A.REF_BLOCK)) and callable(modules.attention_stage(A.REF_STAGE))
    for _, _, _, _, cfg in A.STAGE_CASES.values():
        assert callable((modules.attention_stage if "depth" in cfg else modules.attention_block)(cfg))
    modules.attention_block(dict(GOOD, abs_pos_encoding=True, pos_encoding=None))      # nothing is added
    modules.attention_block(dict(GOOD, ff_factor0=0, ff_factor1=0, ff_kernel_size=0, ff_multiplier=0))
    modules.check_attention_config(GOOD, True, 64)


@pytest.mark.parametrize("bad", [{"dropout_rate": None}, {"dropout_rate": 0.1}, {"pos_encoding": "rff"}, {"pos_encoding": None},
                                 {"pos_encoding": "sinus"}, {"key_dim": 36}, {"key_dim": 72}, {"key_dim": 0}, {"n_head": 0}, {"kernel_size": -1},
                                 {"kernel_size": 65}, {"ff_kernel_size": -1}, {"ff_kernel_size": 0}, {"ff_factor0": -0.5}, {"ff_factor1": -1},
                                 {"ff_factor0": 0, "ff_factor1": 0}, {"ff_factor0": 0, "ff_factor1": 0, "ff_kernel_size": 0},
                                 {"activation": "gelu"}, {"depth": 0}] + [{k: None} for k in ("key_dim", "n_head", "kernel_size", "ff_kernel_size",
                                                                                             "ff_multiplier", "ff_factor0", "ff_factor1", "depth")])
def test_factories_refuse_what_has_no_kernel_or_what_the_reference_refuses(bad):
    """None: the key is removed.  Dropout (absent = the reference's 0.1), the unreproducible random Fourier table, relative positions without a
    table, head widths the kernels do not have, sizes out of range, negative factors, unused FF modules with a kernel size or a multiplier
    (modules.py:540-551), an unknown activation, a missing mandatory key"""
    from seld_amd import modules
    cfg = {k: v for k, v in dict(GOOD, **bad).items() if not (k in bad and bad[k] is None and k != "pos_encoding")}
    with pytest.raises(ValueError):
        modules.attention_stage(cfg)
    if "depth" not in bad:
        with pytest.raises(ValueError):
            modules.attention_block({k: v for k, v in cfg.items() if k != "depth"})


def test_basic_encoding_refuses_an_odd_width_and_first_stays_refused():
    from seld_amd import models, modules
    with pytest.raises(ValueError) as e:
        modules.attention_block(A.REF_BLOCK)((2, 10, 33))
    assert "odd width" in str(e.value)
    with pytest.raises(ValueError):
        modules.attention_block(dict(A.REF_BLOCK, ff_multiplier=0.01))((2, 10, 32))      # int(ff_multiplier * D) = 0
    for first in ("attention_block", "attention_stage"):
        with pytest.raises(ValueError):
            models._arch_from_config({"FIRST": first, "SECOND": "bidirectional_GRU_block", "SED": "simple_dense_block", "DOA": "simple_dense_block"},
                                     7, 64)
    with pytest.raises(ValueError):      # the conformer's relative mode stays refused
        modules.conformer_encoder_block({"dropout_rate": 0, "pos_mode": "relative"})


# ---------------------------------------------------------------- the C entry points
def test_entry_points_refuse_bad_arguments(seld_lib):
    lib = seld_lib
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    fargs = (("Q", p), ("K", p), ("V", p), ("ldq", 16), ("ldk", 16), ("ldv", 16), ("P", p), ("ldp", 16), ("u", p), ("vb", p), ("O", p), ("lse", p),
             ("B", 1), ("S", 2), ("H", 2), ("d", 8), ("scale", 1.0), ("stream", None))
    bargs = (("Q", p), ("K", p), ("V", p), ("ldq", 16), ("ldk", 16), ("ldv", 16), ("P", p), ("ldp", 16), ("u", p), ("vb", p), ("O", p), ("dO", p),
             ("lse", p), ("dQu", p), ("dQv", p), ("dK", p), ("dV", p), ("dP", p), ("lddqu", 16), ("lddqv", 16), ("lddk", 16), ("lddv", 16),
             ("lddp", 16), ("scratch", p), ("B", 1), ("S", 2), ("H", 2), ("d", 8), ("scale", 1.0), ("stream", None))
    fwd = lambda **kw: lib.seld_relattn_fwd(*[kw.get(n, d) for n, d in fargs])
    bwd = lambda **kw: lib.seld_relattn_bwd(*[kw.get(n, d) for n, d in bargs])
    for call, args, optional in ((fwd, fargs, ("lse",)), (bwd, bargs, ())):
        for d in (0, 4, 12, 72, -8):
            assert call(d=d) == UNSUPPORTED and call(d=d, Q=None, B=0) == UNSUPPORTED      # the head width first
        for name, dflt in args:
            if dflt is p and name not in optional:
                assert call(**{name: None}) == INVALID, name
            if name.startswith("ld"):
                assert call(**{name: 15}) == INVALID and call(**{name: -16}) == INVALID, name
        for bad in ({"B": 0}, {"S": 0}, {"H": 0}, {"H": 1 << 29, "d": 8}):      # H d wraps in 32 bits: covered by no stride
            assert call(**bad) == INVALID, bad
        assert call(B=1 << 20, S=1 << 20) == UNSUPPORTED      # the grid
        assert call(S=0x7fffffff) == UNSUPPORTED      # a band index 2 S leaves an int
    for bad in ((2, 5, 2, 12), (0, 5, 2, 8), (2, 0, 2, 8), (2, 5, 0, 8), (1 << 20, 1 << 20, 2, 8), (1, 5, 1 << 29, 8)):
        assert lib.seld_relattn_bwd_scratch(*bad) == -1
    assert lib.seld_relattn_bwd_scratch(3, 100, 4, 16) == 3 * 4 * 100 * 33      # linear in S
    assert lib.seld_relattn_bwd_scratch(32, 600, 4, 24) == 2 * lib.seld_relattn_bwd_scratch(32, 300, 4, 24)
    glu = lambda **kw: lib.seld_glu_fwd(*[kw.get(n, d) for n, d in (("u", p), ("ldu", 8), ("y", p), ("rows", 2), ("C", 4), ("stream", None))])
    glub = lambda **kw: lib.seld_glu_bwd(*[kw.get(n, d) for n, d in (("u", p), ("ldu", 8), ("dy", p), ("du", p), ("lddu", 8), ("rows", 2), ("C", 4),
                                                                   ("stream", None))])
    for call, ptrs in ((glu, ("u", "y")), (glub, ("u", "dy", "du"))):
        for name in ptrs:
            assert call(**{name: None}) == INVALID, name
        for bad in ({"rows": 0}, {"C": 0}, {"ldu": 7}, {"ldu": -8}, {"C": 1 << 30, "ldu": 0x7fffffff}):
            assert call(**bad) == INVALID, bad
        wide = {"lddu": 128} if call is glub else {}
        assert call(rows=1 << 40, C=64, ldu=128, **wide) == UNSUPPORTED
    assert glub(lddu=7) == INVALID


# ---------------------------------------------------------------- the 1e-4 bar applies unchanged
@pytest.mark.parametrize("B,S,H,d", A.RELATTN_CASES)
def test_plain_fp32_relattn_is_within_5e_5_of_fp64(B, S, H, d):
    ins = A.relattn_inputs(B, S, H, d)
    r64, r32 = A.relattn_reference(*ins), A.relattn_reference(*ins, dtype=torch.float32)
    biggest = max(np.abs(r64[n]).max() for n in ("dQu", "dQv", "dK", "dV", "dP"))
    worst = max(rel_err(r32[n], r64[n]) for n in r64 if np.abs(r64[n]).max() >= 1e-9 * biggest)
    print(f"[fp32 vs fp64] relattn {(B, S, H, d)}: {worst:.3e}")
    assert worst <= FP32_CAP


@pytest.mark.parametrize("name", sorted(A.STAGE_CASES))
def test_plain_fp32_evaluation_of_every_gpu_case_is_within_5e_5_of_fp64(name):
    B, S, D, depth, cfg = A.STAGE_CASES[name]
    r64 = A.stage_reference(B, S, D, depth, cfg, seed=3, dtype=torch.float64)
    r32 = A.stage_reference(B, S, D, depth, cfg, seed=3, dtype=torch.float32)
    worst = max(rel_err(r32[key], r64[key]) for key in ("out_train", "out_eval", "dx") + (("new_state",) if r64["specs"][1] else ()))
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


def test_plain_fp32_train_step_of_the_composed_model_is_within_5e_5_of_fp64(seldnet_config):
    from oracle import seldnet_oracle as O
    from test_modules_gpu import STAGE_FIRST
    cfg = A.model_case(seldnet_config, STAGE_FIRST)
    tr, nt = A.variable_specs(cfg, A.MODEL_INPUT)
    assert any(n == "at1.mha.pos_bias_v" for n, _ in tr) and [n for n, _ in nt][-2:] == ["at1.bn.moving_mean", "at1.bn.moving_variance"]
    w, st = A.random_weights(cfg, A.MODEL_INPUT, seed=11)
    x, ys, yd = O.synthetic_batch(*A.MODEL_INPUT[:2], seed=23)
    r64 = A.train_step(cfg, A.MODEL_INPUT, w, st, x, ys, yd)
    r32 = A.train_step(cfg, A.MODEL_INPUT, w, st, x, ys, yd, dtype=torch.float32)
    worst = max(rel_err(r32[k], r64[k]) for k in ("sed", "doa", "sloss", "dloss", "grad", "new_state"))
    print(f"[fp32 vs fp64] composed model: {worst:.3e}")
    assert worst <= FP32_CAP
