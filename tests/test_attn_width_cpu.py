"""The any-width attention (seld_attnw_*, modules' any_key_dim, ConvTemporalNet search=True) and the search's attention stages
(nas_seldnet.search_space_1d_attention, --attention_stages) without a device: the entries' signatures and refusal order (the library loads
without a device; a call that got as far as a launch returns SELD_ERR_HIP there, so the code shows that the refusal came first —
tests/test_module_ops_cpu.py), the configuration rules, the plan of a model with key_dim 6 and 12, and the search space, sampler and
constraint.  Also the fp32 margin of the cases tests/test_attn_width_gpu.py runs (the rule of tests/test_rnn_cpu.py)."""
import copy
import ctypes as C
import re

import numpy as np
import pytest
import torch

import attn_width_cases as A
import conformer_oracle as K
import conv_temporal_oracle as CT
import transformer_oracle as T
from helpers import rel_err

INVALID, UNSUPPORTED, HIP = -1, -2, -3
FP32_MARGIN = 5e-5
_I, _L, _F, _P, _U, _U64 = C.c_int, C.c_int64, C.c_float, C.c_void_p, C.c_uint, C.c_uint64
FWD_SIG = [_P, _P, _P, _I, _I, _I, _P, _P, _I, _I, _I, _I, _F]
BWD_SIG = [_P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _I, _I, _I, _I, _F]
DROP_SIG = [_F, _U64, _U, _U]
SIGS = {"seld_attnw_fwd": (_I, FWD_SIG + [_P]), "seld_attnw_bwd_scratch": (_L, [_I] * 4), "seld_attnw_bwd": (_I, BWD_SIG + [_P]),
        "seld_attnw_drop_fwd": (_I, FWD_SIG + DROP_SIG + [_P]), "seld_attnw_drop_bwd": (_I, BWD_SIG + DROP_SIG + [_P])}


# ---------------------------------------------------------------- the entries
def test_the_five_symbols_exist_with_the_declared_signatures(seld_lib):
    from seld_amd import _lib
    import os
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "seld_hip.h")).read()
    for name, (res, args) in SIGS.items():
        fn = getattr(seld_lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
        twin = name.replace("attnw", "attn")      # the same arguments as the entry it widens
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[twin], name
        decl = lambda n: re.sub(r"\s+", " ", re.search(r"\n(?:int|int64_t) " + n + r"\(([^;]*)\);", header).group(1))
        assert decl(name) == decl(twin), name


@pytest.fixture(scope="module")
def env(seld_lib):
    gpu = torch.cuda.is_available()
    buf = torch.zeros(1 << 12, device="cuda") if gpu else None
    p = C.c_void_p(buf.data_ptr()) if gpu else C.c_void_p(1 << 20)     # no device: never dereferenced, a launch fails first
    yield seld_lib, p, gpu
    del buf


FWD_PTRS, BWD_PTRS = ["Q", "K", "V", "O", "lse"], ["Q", "K", "V", "O", "dO", "lse", "dQ", "dK", "dV", "scratch"]


def _call(env, op, B=1, S=2, H=2, d=3, rate=None, ld=None, **over):
    """the base call [B, S, H, d] on one buffer (every operand the same floats: the values are not looked at); over: a pointer as None, or
    a stride by its name"""
    lib, p, _ = env
    g = lambda n: over.get(n, p)
    s = lambda n: over.get(n, H * d if ld is None else ld)
    tail = ([0.5 if rate is None else rate, 1, 2, 3] if "drop" in op else []) + [None]
    if "fwd" in op:
        return getattr(lib, op)(g("Q"), g("K"), g("V"), s("ldq"), s("ldk"), s("ldv"), g("O"), g("lse"), B, S, H, d, 0.5, *tail)
    return getattr(lib, op)(g("Q"), g("K"), g("V"), s("ldq"), s("ldk"), s("ldv"), g("O"), g("dO"), g("lse"), g("dQ"), g("dK"), g("dV"),
                            s("lddq"), s("lddk"), s("lddv"), g("scratch"), B, S, H, d, 0.5, *tail)


@pytest.mark.parametrize("op", ["seld_attnw_fwd", "seld_attnw_bwd", "seld_attnw_drop_fwd", "seld_attnw_drop_bwd"])
def test_refusal_order_of_the_entries(env, op):
    launched = 0 if env[2] else HIP
    for d in (1, 3, 8, 12, 63, 64):
        assert _call(env, op, d=d) == launched, f"d = {d}: the base call must get as far as its launch"
    if env[2]:
        torch.cuda.synchronize()
    for d in (0, 65, -1):      # the width first, whatever else is wrong
        assert _call(env, op, d=d) == UNSUPPORTED
        assert _call(env, op, d=d, Q=None) == UNSUPPORTED
        assert _call(env, op, d=d, B=0) == UNSUPPORTED
        assert _call(env, op, d=d, ld=0) == UNSUPPORTED
        if "drop" in op:
            assert _call(env, op, d=d, rate=1.5) == UNSUPPORTED
    ptrs = FWD_PTRS if "fwd" in op else BWD_PTRS
    for n in ptrs:
        if "fwd" in op and n == "lse":      # NULL at inference
            assert _call(env, op, lse=None) == launched
        else:
            assert _call(env, op, **{n: None}) == INVALID, n
    for n in ["ldq", "ldk", "ldv"] + ([] if "fwd" in op else ["lddq", "lddk", "lddv"]):
        assert _call(env, op, **{n: 5}) == INVALID, n      # H d = 6
        assert _call(env, op, **{n: 7}) == launched, n      # an odd stride is a stride
    for bad in ({"B": 0}, {"S": 0}, {"H": 0}, {"B": -1}):
        assert _call(env, op, **bad) == INVALID, bad
    if "drop" in op:
        for r in (-0.1, 1.0, 1.5, float("nan")):
            assert _call(env, op, rate=r) == INVALID, r
        assert _call(env, op, rate=0.0) == launched
        assert _call(env, op, B=1 << 20, S=1 << 6, H=1 << 7, ld=1 << 9, d=3, rate=0.5) == UNSUPPORTED      # B H S = 2^33 at rate > 0
    assert _call(env, op, B=1 << 20, S=1, H=1 << 12, ld=1 << 14, d=3) == UNSUPPORTED      # the grid B H ceil(S / 64) = 2^32


def test_scratch_sizes(seld_lib):
    for d in (0, 65, -1):
        assert seld_lib.seld_attnw_bwd_scratch(2, 5, 3, d) == -1 and seld_lib.seld_attnw_bwd_scratch(0, 5, 3, d) == -1
    for d in (1, 3, 8, 12, 63, 64):
        assert seld_lib.seld_attnw_bwd_scratch(2, 5, 3, d) == 2 * 5 * 3
        assert seld_lib.seld_attnw_bwd_scratch(0, 5, 3, d) == -1 and seld_lib.seld_attnw_bwd_scratch(2, 0, 3, d) == -1
    assert seld_lib.seld_attn_bwd_scratch(2, 5, 3, 12) == -1      # the narrow entries keep refusing what is no multiple of 8


# ---------------------------------------------------------------- configuration rules
TF = {"n_head": 2, "ff_multiplier": 2, "kernel_size": 3, "dropout_rate": 0}
CF = {"n_head": 2, "kernel_size": 4, "multiplier": 2, "pos_encoding": None, "dropout_rate": 0}


def test_any_key_dim_config_rules():
    from seld_amd.modules import _check_second, check_conformer_config, check_transformer_config
    for dk in (1, 3, 12, 63, 8, 64, np.int64(6)):
        check_transformer_config(dict(TF, key_dim=dk), any_key_dim=True)
        check_transformer_config(dict(TF, key_dim=dk, depth=2), True, any_key_dim=True)
        check_conformer_config(dict(CF, key_dim=dk), any_key_dim=True)
        check_conformer_config(dict(CF, key_dim=dk, depth=1), True, D=16, any_key_dim=True)
        _check_second("transformer_encoder_block", dict(TF, key_dim=dk), None, False, False, True)
        _check_second("conformer_encoder_stage", dict(CF, key_dim=dk, depth=1), 16, False, False, True)
    for dk in (0, 65, 2.5, True, -3, "12", None):
        with pytest.raises(ValueError, match="from 1 to 64"):
            check_transformer_config(dict(TF, key_dim=dk), any_key_dim=True)
        with pytest.raises(ValueError, match="from 1 to 64"):
            check_conformer_config(dict(CF, key_dim=dk), any_key_dim=True)
    # without the keyword: today's refusal, in today's words
    for dk in (3, 12, 63, 4):
        msg = f"^key_dim {dk}: the attention kernels take a multiple of 8 from 8 to 64$"
        with pytest.raises(ValueError, match=msg):
            check_transformer_config(dict(TF, key_dim=dk))
        with pytest.raises(ValueError, match=msg):
            check_conformer_config(dict(CF, key_dim=dk))
        with pytest.raises(ValueError, match=msg):
            _check_second("transformer_encoder_block", dict(TF, key_dim=dk), None, False, True)      # any_units is not any_key_dim
    # attention_block is in neither search space: multiples of 8 with or without a search runtime (relattn.hip)
    from seld_amd.modules import check_attention_config
    import inspect
    assert "any_key_dim" not in inspect.signature(check_attention_config).parameters


def test_the_plan_of_a_model_with_key_dim_6_and_12():
    from seld_amd import models
    from seld_amd.modules import ConvTemporalNet
    cfg, shape = A.CONFIG, A.INPUT
    tr, nt = CT.variable_specs(cfg, shape)
    m = models.conv_temporal(shape, cfg, "meta", search=True)
    assert m.rt.any_key_dim and m.rt.any_units
    assert [(n, s) for n, _, s in m.variables] == tr and [(n, s) for n, _, s in m.state_variables] == nt
    shapes = {n: s for n, _, s in m.variables}
    D = 16
    for part in ("query", "key", "value"):
        assert shapes[f"b0.tf0.mha.{part}.kernel"] == (D, 2, 6) and shapes[f"b0.tf0.mha.{part}.bias"] == (2, 6)
        assert shapes[f"sed.cf0.mha.{part}_kernel"] == (2, D, 12)      # the reference's own layer: head-major
    assert shapes["b0.tf0.mha.attention_output.kernel"] == (2, 6, D) and shapes["sed.cf0.mha.projection_kernel"] == (2, 12, D)
    assert m.body[0].blocks[0].mha.wide and m.heads[0].body.blocks[0].mha.wide
    cx = m.complexity()
    assert cx["params"] == sum(int(np.prod(s)) for _, s in tr) and cx["flops"] > 0
    for build in (lambda: ConvTemporalNet(shape, cfg, "meta"), lambda: models.conv_temporal(shape, cfg, "meta"),
                  lambda: models.conv_temporal(shape, cfg, "meta", search=False)):
        with pytest.raises(ValueError, match="key_dim 6: the attention kernels take a multiple of 8"):
            build()
    # a multiple of 8 on the search runtime keeps the narrow entries
    cfg8 = copy.deepcopy(cfg)
    cfg8["BLOCK0_ARGS"]["key_dim"] = 8
    assert not models.conv_temporal(shape, cfg8, "meta", search=True).body[0].blocks[0].mha.wide
    # complexity: the projections' width follows H dk, a multiple of nothing (params; the count of products is the Linear layers' alone)
    cfg7 = copy.deepcopy(cfg)
    cfg7["BLOCK0_ARGS"]["key_dim"] = 7
    more = models.conv_temporal(shape, cfg7, "meta", search=True).complexity()
    assert more["params"] - cx["params"] == (4 * D * 2 + 3 * 2) * (7 - 6), "three projections in with their biases and one out, H = 2"
    assert more["flops"] == cx["flops"]


# ---------------------------------------------------------------- fp32 margin of the GPU cases
@pytest.mark.parametrize("d,S", A.PARITY_CASES)
def test_fp32_margin_of_the_kernel_cases(d, S):
    r64, r32 = A.reference(S, d), A.reference(S, d, torch.float32)
    biggest = max(np.abs(r).max() for r in r64[2:])
    for name, a, b in zip(A.NAMES, r32, r64):
        if np.abs(b).max() < 1e-9 * biggest:      # S = 1: dQ = dK = 0 by mathematics
            assert np.abs(a).max() <= 1e-3 * biggest
        else:
            assert rel_err(a, b) <= FP32_MARGIN, (d, S, name)


def test_fp32_margin_of_the_block_and_model_cases():
    from oracle import seldnet_oracle as O
    B, S, D, cfg = A.TRANSFORMER_BLOCK
    specs = T.stage_specs(D, cfg, 1)
    w = T.random_block_weights(specs, 3)
    x = T.f32(np.random.default_rng(3).standard_normal((B, S, D)))
    y = [T.stage_forward(torch.tensor(x, dtype=dt), O.unflatten(torch.tensor(w, dtype=dt), specs), cfg, 1).numpy()
         for dt in (torch.float32, torch.float64)]
    assert rel_err(y[0], y[1]) <= FP32_MARGIN
    B, S, D, cfg = A.CONFORMER_BLOCK
    a, b = K.stage_reference(B, S, D, 1, cfg, 3, torch.float32), K.stage_reference(B, S, D, 1, cfg, 3)
    for k in ("out_train", "out_eval", "dx", "grad"):
        assert rel_err(a[k], b[k]) <= FP32_MARGIN, k
    w, st, x, ys, yd, ref = A.model_reference()
    r32 = CT.train_step(A.CONFIG, A.INPUT, w, st, x, ys, yd, doa_loss="MSE", loss_weight=(1.0, 1000.0), lr=1e-3, step=1, dtype=torch.float32)
    for k in ("sed", "doa", "grad"):
        assert rel_err(r32[k], ref[k]) <= FP32_MARGIN, k


# ---------------------------------------------------------------- the search
def test_attention_search_space_holds_the_reference_values():
    from seld_amd import nas_seldnet as N
    key_dim = [2, 3, 4, 6, 8, 12, 16, 24, 32, 48]
    assert N.search_space_1d_attention == {
        "transformer_encoder_stage": {"depth": [1, 2, 3], "n_head": [1, 2, 4, 8, 16], "key_dim": key_dim,
                                      "ff_multiplier": [0.25, 0.5, 1, 2, 4, 8], "kernel_size": [1, 3, 5]},
        "conformer_encoder_stage": {"depth": [1, 2, 3], "key_dim": key_dim, "n_head": [1, 2, 4, 8, 16],
                                    "kernel_size": [4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256], "multiplier": [1, 2, 4],
                                    "pos_encoding": [None, "basic", "rff"]}}
    assert key_dim == A.SEARCH_KEY_DIMS
    for kind, space in N.search_space_1d_attention.items():      # the reference's order of kinds and of arguments: the draws follow it
        assert list(space) == {"transformer_encoder_stage": ["depth", "n_head", "key_dim", "ff_multiplier", "kernel_size"],
                               "conformer_encoder_stage": ["depth", "key_dim", "n_head", "kernel_size", "multiplier", "pos_encoding"]}[kind]
    N.search_space_sanity_check(N.search_space_1d_attention)
    assert not set(N.search_space_1d) & set(N.search_space_1d_attention)
    assert N.get_parser().parse_args(["--name", "x"]).attention_stages is False
    assert N.get_parser().parse_args(["--name", "x", "--attention_stages"]).attention_stages is True


def _key_dim_cases():
    for kind in ("transformer_encoder_stage", "conformer_encoder_stage"):
        for dk in A.SEARCH_KEY_DIMS:
            yield kind, dk


@pytest.mark.parametrize("kind,dk", list(_key_dim_cases()))
def test_constraint_accepts_every_key_dim_of_the_space(kind, dk):
    """as BLOCK0 and as both heads, on the meta device (half of the values could not be built before seld_attnw_* and search=True)"""
    from seld_amd import nas_seldnet as N
    args = {k: v[0] for k, v in N.search_space_1d_attention[kind].items()}
    args["key_dim"] = dk
    cfg = {"n_classes": 12, "BLOCK0": kind, "BLOCK0_ARGS": dict(args), "SED": kind, "SED_ARGS": dict(args), "DOA": kind, "DOA_ARGS": dict(args)}
    assert N.sample_constraint()(N.postprocess_fn(cfg), [2, 300, 64, 7])


def test_constraint_rejects_what_has_no_kernel():
    from seld_amd import nas_seldnet as N
    head = {"depth": 1, "units": 8}
    cf = {"depth": 1, "key_dim": 6, "n_head": 2, "kernel_size": 4, "multiplier": 1, "pos_encoding": None}
    mk = lambda **kw: {"n_classes": 12, "BLOCK0": "conformer_encoder_stage", "BLOCK0_ARGS": dict(cf, **kw), "SED": "bidirectional_GRU_stage",
                       "SED_ARGS": dict(head), "DOA": "bidirectional_GRU_stage", "DOA_ARGS": dict(head)}
    ok = N.sample_constraint()
    even = odd = [2, 300, 64, 7]      # the width behind the stem is even: the odd one comes from a GRU stage in front
    assert ok(mk(), even) and ok(mk(kernel_size=64), even) and ok(mk(pos_encoding="basic"), even)
    assert not ok(mk(kernel_size=96), even) and not ok(mk(kernel_size=256), even)
    assert not ok(mk(pos_encoding="rff"), even)
    behind_odd = mk(pos_encoding="basic")
    behind_odd["BLOCK1"], behind_odd["BLOCK1_ARGS"] = behind_odd["BLOCK0"], behind_odd["BLOCK0_ARGS"]
    behind_odd["BLOCK0"], behind_odd["BLOCK0_ARGS"] = "bidirectional_GRU_stage", {"depth": 1, "units": 5}
    assert not ok(behind_odd, odd), "'basic' on an odd width"
    behind_odd["BLOCK0_ARGS"]["units"] = 6
    assert ok(behind_odd, odd)


SAMPLER_SEED, MAX_TRIES, N_DRAWS = 0, 200, 12


def test_sampler_with_attention_stages_returns_only_buildable_configurations():
    """the seeded draws of --attention_stages' space under sample_constraint(): every returned configuration plans, none holds a conformer
    kernel above 64 taps or 'rff', attention stages with a key_dim that is no multiple of 8 are among them, and no draw needs more than
    MAX_TRIES rejections (chosen here: the largest count seen is printed)"""
    from seld_amd import nas_seldnet as N
    space = {**N.search_space_1d, **N.search_space_1d_attention}
    assert list(space) == list(N.search_space_1d) + list(N.search_space_1d_attention)
    rng = np.random.default_rng(SAMPLER_SEED)
    tries, kinds, ragged = [], set(), set()
    inner = N.sample_constraint()

    def counted(c, s):
        tries[-1] += 1
        return inner(c, s)
    for _ in range(N_DRAWS):
        tries.append(0)
        c = N.conv_temporal_sampler(N.search_space_2d, space, 4, [2, 300, 64, 7], {"n_classes": 12}, N.postprocess_fn, counted, rng, MAX_TRIES)
        N.plan(c, [2, 300, 64, 7])      # buildable: raises otherwise
        for key in [k for k in c if k.startswith("BLOCK") and not k.endswith("_ARGS")] + ["SED", "DOA"]:
            kind, a = c[key], c[f"{key}_ARGS"]
            kinds.add(kind)
            if kind == "conformer_encoder_stage":
                assert a["kernel_size"] <= 64 and a["pos_encoding"] in (None, "basic"), a
            if kind in N.search_space_1d_attention:
                assert a["key_dim"] in A.SEARCH_KEY_DIMS
                if a["key_dim"] % 8:
                    ragged.add(a["key_dim"])
    print(f"draws per accepted configuration: {tries}")
    assert max(tries) <= MAX_TRIES // 4, "MAX_TRIES leaves no room"
    assert set(N.search_space_1d_attention) <= kinds, kinds
    assert ragged, "no draw reached a key_dim that needs seld_attnw_*"
