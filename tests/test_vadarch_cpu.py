"""models.vad_architecture without a device: the configuration rules on torch's `meta` device (modules.VadArchNet(..., device='meta'): every
layer is constructed, nothing is allocated or run), complexity() on a hand-counted configuration, the sampler, postprocess_fn and the
constraint of seld_amd/nas_vad.py, the head kernels' refusals that come before anything is enqueued, and the pieces of
tests/vadarch_oracle.py the device tests lean on."""
import ctypes as C

import numpy as np
import pytest

import vadarch_oracle as VO

INVALID, UNSUPPORTED = -1, -2
SHAPE = (4, 7, 80, 1)
MOTHER = {"filters0": 0, "filters1": 6, "filters2": 0, "kernel_size0": 0, "kernel_size1": 3, "kernel_size2": 0, "connect0": [1],
          "connect1": [1, 0], "connect2": [0, 0, 1], "strides": [1, 2]}
DENSE = {"depth": 1, "units": 8}


def plan(cfg, shape=SHAPE, **kw):
    from seld_amd import modules
    return modules.VadArchNet(shape, cfg, "meta", **kw)


def test_reference_test_configs_give_window_predictions():
    """models_test.py::test_vad_architecture: both configurations predict [B, 7]; Dense on the 2-D tensor, Conv1D on the 3-D one"""
    a, b = (plan(c) for c in VO.REF_TEST_CONFIGS)
    assert a.output_shape() == b.output_shape() == (4, 7) and a.output_shape(2) == (2, 7)
    assert [(n, sh) for n, _, sh in a.variables] == [("b0.dense0.kernel", (560, 512)), ("b0.dense0.bias", (512,)), ("b0.dense1.kernel", (512, 512)),
                                                     ("b0.dense1.bias", (512,)), ("out.kernel", (512, 7)), ("out.bias", (7,))]
    assert [(n, sh) for n, _, sh in b.variables] == [("b0.dense0.kernel", (1, 80, 512)), ("b0.dense0.bias", (512,)), ("b0.dense1.kernel", (1, 512, 512)),
                                                     ("b0.dense1.bias", (512,)), ("out.kernel", (512, 1)), ("out.bias", (1,))]
    assert a.state_variables == b.state_variables == []
    # simple_dense_stage overwrites dense_activation with the absent `activation`: linear layers; the Dropout rate is the block's
    from seld_amd.modules import ACT, DROP_STREAM0
    assert a.body[0].act == ACT[None] and a.body[0].drop.rate == 0.5 and a.body[0].drop.base == DROP_STREAM0
    assert a.fused and b.fused and not plan(VO.REF_TEST_CONFIGS[0], fused_head=False).fused


@pytest.mark.parametrize("name", ["a", "b"])
def test_variables_match_the_oracle(name):
    cfg, shape = VO.MODEL_CASES[name]
    m = plan(cfg, shape)
    tr, nt = VO.variable_specs(cfg, shape)
    assert [(n, sh) for n, _, sh in m.variables] == [(n, tuple(sh)) for n, sh in tr]
    assert [(n, sh) for n, _, sh in m.state_variables] == [(n, tuple(sh)) for n, sh in nt]
    assert m.output_shape() == (shape[0],) + VO.walk(cfg, shape)[3]


BAD = [
    (dict(flatten=True, BLOCK0="mother_stage", BLOCK0_ARGS=dict(MOTHER, depth=1)), "flatten has made the input 2-D"),
    (dict(flatten=True, BLOCK0="RNN_block", BLOCK0_ARGS={"units": 128}), "needs a time axis"),
    (dict(flatten=False, BLOCK0="simple_dense_stage", BLOCK0_ARGS=DENSE, BLOCK1="mother_block", BLOCK1_ARGS=MOTHER), "has made it 3-D"),
    (dict(flatten=False, BLOCK0="simple_dense_stage"), "vad_architecture: BLOCK0 has no BLOCK0_ARGS"),
    (dict(flatten=False, BLOCK0="res_basic_stage", BLOCK0_ARGS={}), "vad_architecture: BLOCK0 = 'res_basic_stage'"),
    (dict(flatten=True, last_unit=0), "last_unit"),
    (dict(flatten=True, BLOCK0="simple_dense_stage", BLOCK0_ARGS=dict(DENSE, dropout_rate=1.0)), "0 <= dropout_rate < 1"),
]


@pytest.mark.parametrize("cfg,msg", BAD)
def test_configuration_errors(cfg, msg):
    with pytest.raises(ValueError, match=msg):
        plan(cfg)


def test_bad_input_shape_and_fused_head_width():
    with pytest.raises(ValueError, match="input_shape"):
        plan({}, (7, 80, 1))
    with pytest.raises(ValueError, match="fused head"):
        plan({"last_unit": 9}, fused_head=True)
    assert not plan({"last_unit": 9}).fused and plan({"last_unit": 8}).fused


def test_blocks_are_sorted_as_strings():
    cfg = {"flatten": True, "BLOCK2": "simple_dense_stage", "BLOCK2_ARGS": {"depth": 1, "units": 5},
           "BLOCK10": "simple_dense_stage", "BLOCK10_ARGS": {"depth": 1, "units": 3}}
    m = plan(cfg)
    assert [(n, sh) for n, _, sh in m.variables][:4] == [("b0.dense0.kernel", (560, 3)), ("b0.dense0.bias", (3,)), ("b1.dense0.kernel", (3, 5)),
                                                         ("b1.dense0.bias", (5,))]      # BLOCK10 comes first: index 0


def test_dense_block_refuses_dropout_unless_wired():
    from seld_amd import modules
    with pytest.raises(ValueError, match="dropout_rate must be 0"):
        modules.check_dense_config({"units": [8], "dropout_rate": 0.2})
    assert modules.check_dense_config({"units": [8], "dropout_rate": 0.2}, dropout=True) == float(np.float32(0.2))
    assert modules.check_dense_config({"units": [8]}) == 0.0
    with pytest.raises(ValueError, match="dropout_rate must be 0"):      # the refusal compares the value as given, not its fp32 rounding
        modules.check_dense_config({"units": [8], "dropout_rate": 1e-60})
    import torch
    rt = modules._Rt(torch.device("meta"))
    with pytest.raises(ValueError, match="dropout_rate must be 0"):
        modules.DenseBlock(rt, {"units": [8], "dropout_rate": 0.2}, 7, 80, "d", 2)
    blk = modules.DenseBlock(rt, {"units": [8, 4], "dropout_rate": 0.2}, 7, 80, "d", 2, dropout=True, first_block=3)
    assert blk.drop.base == modules.DROP_STREAM0 + 96 and blk.out_dim == 4
    # the chain of models.conv_temporal keeps its refusal (tests/test_conv_temporal_cpu.py pins the message)
    assert modules.ConvTemporalNet.DENSE_KW == {}


def test_dropout_streams_count_the_blocks_in_front():
    from seld_amd.modules import DROP_STREAM0
    cfg = dict(VO.CFG_B, BLOCK1_ARGS=dict(VO.CFG_B["BLOCK1_ARGS"], dropout_rate=0.2))
    m = plan(cfg, VO.MODEL_CASES["b"][1])
    assert len(m.blocks) == 2 and m.body[0].drop.base == DROP_STREAM0 + 64      # two mother blocks in front
    assert VO.walk(cfg, VO.MODEL_CASES["b"][1])[2][-1][3] == 2


def test_complexity_counts_the_dense_products_per_window():
    # flatten: 560 -> 8 -> 8 -> 7
    m = plan({"flatten": True, "last_unit": 7, "BLOCK0": "simple_dense_stage", "BLOCK0_ARGS": {"depth": 2, "units": 8}})
    assert m.complexity() == {"flops": 560 * 8 + 8 * 8 + 8 * 7, "params": 560 * 8 + 8 + 8 * 8 + 8 + 8 * 7 + 7}
    # [7, 80, 1]: a 3 x 3 convolution 1 -> 6 with strides (1, 2) on 7 x 40 outputs and its 1 x 1 strided projection, the output the
    # concatenation of the second layer alone; Conv1D 240 -> 8 on 7 frames; Dense(1) on 7 frames
    cfg = {"flatten": False, "last_unit": 1, "BLOCK0": "mother_block", "BLOCK0_ARGS": MOTHER, "BLOCK1": "simple_dense_stage", "BLOCK1_ARGS": DENSE}
    m = plan(cfg)
    conv, proj = 7 * 40 * 9 * 6, 7 * 40 * 1 * 6
    assert m.complexity()["flops"] == conv + proj + 7 * 240 * 8 + 7 * 8 * 1
    assert m.complexity()["params"] == m.n_params == (9 * 6 + 6 + 12) + (6 + 6 + 12) + (240 * 8 + 8) + (8 + 1)
    assert plan(cfg, (1, 7, 80, 1)).complexity() == m.complexity()      # per window: the batch does not enter


# ---------------------------------------------------------------- nas_vad
def test_search_spaces_hold_the_reference_values():
    from seld_amd import nas_vad as N
    ms, ds = N.search_space_2d["mother_stage"], N.search_space_1d["simple_dense_stage"]
    assert list(N.search_space_2d) == ["mother_stage"] and list(N.search_space_1d) == ["simple_dense_stage"]
    assert ms["filters0"] == ms["filters1"] == ms["filters2"] and ms["filters0"].count(0) == 11 and ms["filters0"][11:] == ds["units"]
    assert ds["units"] == [3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256] and ms["depth"] == ds["depth"] == [1, 2, 3]
    assert ms["connect2"] == [[0, 0, 0], [0, 0, 1], [0, 1, 0], [0, 1, 1], [1, 0, 0], [1, 0, 1], [1, 1, 0], [1, 1, 1]]
    assert ms["strides"] == [(1, 1), (1, 2), (1, 3)] and ds["dropout_rate"] == [0., 0.2, 0.5] and ds["dense_activation"] == [None, "relu"]
    N.search_space_sanity_check(N.search_space_2d)
    N.search_space_sanity_check(N.search_space_1d)


def test_sanity_check_errors():
    from seld_amd import nas_vad as N
    with pytest.raises(ValueError, match="must be tuple or list"):
        N.search_space_sanity_check({"blk": {"units": 3}})
    with pytest.raises(ValueError, match="must be > 0"):
        N.search_space_sanity_check({"blk": {"units": []}})
    with pytest.raises(ValueError, match="must be tuple or list"):
        N.vad_architecture_sampler(N.search_space_2d, {"blk": {"units": 3}}, 3, [7, 80, 1])


def test_postprocess_rewrites():
    from seld_amd import nas_vad as N
    base = {"depth": 1, "kernel_size0": 3, "kernel_size1": 5, "kernel_size2": 1, "connect0": [1], "connect1": [1, 1], "connect2": [1, 1, 0],
            "strides": (1, 2)}
    go = lambda **f: N.postprocess_fn({"BLOCK0": "mother_stage", "BLOCK0_ARGS": dict(base, **f), "BLOCK1": "simple_dense_stage",
                                       "BLOCK1_ARGS": {"units": 4}})
    # the last layer skipped behind an active second one: the second one is handed on
    a = go(filters0=4, filters1=6, filters2=0)["BLOCK0_ARGS"]
    assert a["connect2"] == [1, 1, 1] and a["kernel_size2"] == 0 and a["kernel_size1"] == 5 and tuple(a["strides"]) == (1, 2)
    # the last two skipped: the first one is handed on, no strides, nothing links to the second
    a = go(filters0=4, filters1=0, filters2=0)["BLOCK0_ARGS"]
    assert a["connect2"] == [1, 1, 0] and a["kernel_size1"] == a["kernel_size2"] == 0 and a["strides"] == [1, 1]
    # the first skipped: nothing links to it
    a = go(filters0=0, filters1=6, filters2=8)["BLOCK0_ARGS"]
    assert a["kernel_size0"] == 0 and a["connect1"] == [1, 0] and a["connect2"] == [1, 0, 0]
    # the argument is not modified and other kinds pass through
    cfg = {"BLOCK0": "mother_stage", "BLOCK0_ARGS": dict(base, filters0=0, filters1=0, filters2=0)}
    before = repr(cfg)
    out = N.postprocess_fn(cfg)
    assert repr(cfg) == before and out["BLOCK0_ARGS"]["connect2"] == [1, 0, 0]
    assert go(filters0=1, filters1=1, filters2=1)["BLOCK1_ARGS"] == {"units": 4}


def test_constraint_windows_and_unbuildable_configurations():
    from seld_amd import nas_vad as N
    cfg = {"flatten": False, "last_unit": 1, "BLOCK0": "simple_dense_stage", "BLOCK0_ARGS": {"depth": 1, "units": 8}}
    flops, params = 7 * 80 * 8 + 7 * 8, 80 * 8 + 8 + 8 + 1
    assert N.plan(cfg, [7, 80, 1]).complexity() == {"flops": flops, "params": params}
    assert N.sample_constraint()(cfg, [7, 80, 1]) and N.sample_constraint(flops, flops, params, params)(cfg, [7, 80, 1])
    assert not N.sample_constraint(min_flops=flops + 1)(cfg, [7, 80, 1]) and not N.sample_constraint(max_flops=flops - 1)(cfg, [7, 80, 1])
    assert not N.sample_constraint(min_params=params + 1)(cfg, [7, 80, 1]) and not N.sample_constraint(max_params=params - 1)(cfg, [7, 80, 1])
    # a ValueError from the plan (nothing reaches the second layer) is a rejection, not a crash
    bad = {"flatten": False, "BLOCK0": "mother_stage", "BLOCK0_ARGS": dict(MOTHER, depth=1, connect0=[0], filters1=6, filters2=4, kernel_size2=1)}
    with pytest.raises(ValueError):
        N.plan(bad, [7, 80, 1])
    assert not N.sample_constraint()(bad, [7, 80, 1])
    # the degenerate mother_stages the reference excludes: one convolution that is not the second; two with an unstrided second
    one = dict(MOTHER, depth=1, filters1=0, kernel_size1=0, filters2=4, kernel_size2=1, connect1=[1, 0], connect2=[0, 0, 0], strides=[1, 1])
    assert not N.sample_constraint()({"flatten": False, "BLOCK0": "mother_stage", "BLOCK0_ARGS": one}, [7, 80, 1])
    two = dict(MOTHER, depth=1, filters2=4, kernel_size2=1, strides=[1, 1])
    assert not N.sample_constraint()({"flatten": False, "BLOCK0": "mother_stage", "BLOCK0_ARGS": two}, [7, 80, 1])


def test_two_hundred_draws_build_or_are_rejected():
    """every raw draw from the nas_vad spaces passes postprocess_fn and then either builds a meta plan or is rejected by the constraint"""
    from seld_amd import nas_vad as N
    rng = np.random.default_rng(2021)
    constraint = N.sample_constraint(20_000, 50_000_000)
    total = {**N.search_space_2d, **N.search_space_1d}
    accepted = 0
    for _ in range(200):
        n_2d = int(rng.integers(0, 4))
        cfg = {"flatten": False, "last_unit": 1}
        for i in range(3):
            kind = "mother_stage" if i < n_2d else "simple_dense_stage"
            cfg[f"BLOCK{i}"], cfg[f"BLOCK{i}_ARGS"] = kind, {k: N._pick(rng, v) for k, v in total[kind].items()}
        cfg = N.postprocess_fn(cfg)
        if constraint(cfg, [7, 80, 1]):
            m = N.plan(cfg, [7, 80, 1])
            assert m.output_shape() == (1, 7) and 20_000 <= m.complexity()["flops"] <= 50_000_000
            accepted += 1
    assert 10 <= accepted < 200      # both outcomes occur
    # and the sampler itself: the same generator gives the same configuration, which the constraint accepts
    draw = lambda: N.vad_architecture_sampler(N.search_space_2d, N.search_space_1d, 3, [7, 80, 1], {"flatten": False, "last_unit": 1},
                                              N.postprocess_fn, constraint, np.random.default_rng(5))
    a, b = draw(), draw()
    assert a == b and constraint(a, [7, 80, 1]) and sorted(k for k in a if k.startswith("BLOCK")) == [f"BLOCK{i}{s}" for i in range(3) for s in ("", "_ARGS")]
    with pytest.raises(RuntimeError, match="no configuration"):
        N.vad_architecture_sampler(N.search_space_2d, N.search_space_1d, 3, [7, 80, 1], constraint=lambda c, s: False, rng=rng, max_tries=3)


def test_train_vad_baseline_knows_both_models():
    from seld_amd import train_vad_baseline as T
    assert tuple(T.MODELS) == ("spectro_temporal_attention_based_VAD", "vad_architecture")
    with pytest.raises(ValueError, match="one of"):
        T.train_and_eval({}, SHAPE, [], [], model="bdnn")


# ---------------------------------------------------------------- the head kernels' refusals (nothing is enqueued: no device needed)
def refusal_checks(lib, p):
    """p: any non-NULL pointer value"""
    fwd, bwd = lib.seld_vadarch_head_fwd, lib.seld_vadarch_head_bwd
    assert fwd(p, p, p, p, 4, 8, 9, None) == UNSUPPORTED and bwd(*[p] * 9, 4, 8, 9, 1.0, None) == UNSUPPORTED
    for i in range(4):
        args = [p] * 4
        args[i] = None
        assert fwd(*args, 4, 8, 1, None) == INVALID
    for i in (0, 1, 2, 3, 4, 6, 7, 8):      # x, w, p, y, loss, dw, db, scratch; dx (5) alone may be NULL: tests/test_vadarch_gpu.py runs that form
        args = [p] * 9
        args[i] = None
        assert bwd(*args, 4, 8, 1, 1.0, None) == INVALID
    for rows, D, U in ((0, 8, 1), (4, 0, 1), (4, 8, 0), (-1, 8, 1)):
        assert fwd(p, p, p, p, rows, D, U, None) == INVALID and bwd(*[p] * 9, rows, D, U, 1.0, None) == INVALID
        assert lib.seld_vadarch_head_bwd_scratch(rows, D, U) == -1
    assert lib.seld_vadarch_head_bwd_scratch(4, 8, 9) == -1
    assert fwd(p, p, p, p, 2 ** 40, 1, 1, None) == UNSUPPORTED      # 2^32 workgroups of 256 rows


def test_head_refusals_come_before_any_launch(seld_lib):
    refusal_checks(seld_lib, C.c_void_p(4096))      # the pointer is never followed: every call is refused on its arguments


def test_head_scratch_sizes(seld_lib):
    f = seld_lib.seld_vadarch_head_bwd_scratch
    assert f(1, 1, 1) == 3 and f(32, 5, 2) == 10 + 1 + 2 and f(33, 5, 2) == 2 * 13 and f(1792, 80, 1) == 56 * 82
    assert f(2 ** 30, 3, 1) == 1024 * 5      # at most 1024 chunks


def test_head_scratch_never_falls_as_rows_grow(seld_lib):
    """a model sizes the scratch once, for its largest batch, and runs every smaller one on it — across the cap of 1024 chunks too
    (rows > 32768), where a count derived from the rounded rows per chunk would rise again for smaller batches"""
    f = seld_lib.seld_vadarch_head_bwd_scratch
    sizes = [f(r, 3, 2) for r in range(1, 70001)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert sizes[32768 - 1] == sizes[-1] == 1024 * (6 + 1 + 2) and sizes[32736 - 1] == 1023 * 9
    for R, smaller in ((35000, (33600, 32767, 32769)), (5000 * 7, (4800 * 7, 4681 * 7)), (2 ** 31 - 1, (2 ** 20, 35000))):
        assert all(f(r, 80, 1) <= f(R, 80, 1) for r in smaller)
    # and the model's buffer is the one of its largest batch
    m = plan({"flatten": False, "last_unit": 1}, (5000, 7, 80, 1))
    assert m.head_scratch.numel() == f(35000, 80, 1) >= max(f(7 * b, 80, 1) for b in (4681, 4800, 4999))


# ---------------------------------------------------------------- the oracle's own pieces
def test_oracle_head_gradients_against_autograd():
    import torch
    x, w, b, y = VO.head_inputs(9, 13, 3)
    ref = VO.head_reference(x, w, b, y, 0.75)
    tx, tw, tb = (torch.tensor(a, requires_grad=True) for a in (x, w, b))
    loss = 0.75 * VO.bce(torch.tensor(y), torch.sigmoid(tx @ tw + tb))
    gx, gw, gb = torch.autograd.grad(loss, (tx, tw, tb))
    assert abs(float(loss.detach()) - ref["loss"]) < 1e-12
    for got, want in ((ref["dx"], gx), (ref["dw"], gw), (ref["db"], gb)):
        assert np.abs(got - want.numpy()).max() < 1e-12 * max(1.0, np.abs(got).max())


def test_oracle_saturated_logits():
    x, w, b, y = VO.saturated_inputs()
    p32 = VO.f32(VO.head_forward(x, w, b))
    assert p32[0, 0] == 1.0 and p32[1, 0] == 1.0 and p32[0, 1] < 1e-7 and p32[1, 1] < 1e-7      # what fp32 holds of sigmoid(+-40)
    loss, dz, *_ = VO.head_backward(x, w, p32, y)
    assert np.isfinite(loss) and (dz[:2] == 0).all() and (dz[2:] != 0).all()


@pytest.mark.parametrize("name", ["a", "b"])
def test_model_cases_keep_their_relu_margin(name):
    cfg, shape, w, st, x, y, _ = VO.model_case(name)
    taps = []
    VO.train_step(cfg, shape, w, st, x, y, taps=taps)
    assert len(taps) >= 2 and VO.relu_margin(taps) >= VO.MARGIN
    if name != "a":
        return
    # fp32 arithmetic stays well inside the bar the device is held to (the dense chain; the mother blocks' room is tests/test_modules_cpu.py's)
    import torch
    r64, r32 = VO.train_step(cfg, shape, w, st, x, y), VO.train_step(cfg, shape, w, st, x, y, dtype=torch.float32)
    from helpers import rel_err
    assert rel_err(r32["pred"], r64["pred"]) < 5e-5 and rel_err(r32["grad"], r64["grad"]) < 5e-5


def test_dropout_masks_enter_the_oracle_forward():
    cfg, shape, w, st, x, y, _ = VO.model_case("a_drop")
    r0, r1, plain = (VO.train_step(cfg, shape, w, st, x, y, step=s) for s in (0, 1, None))
    assert np.abs(r0["pred"] - r1["pred"]).max() > 1e-3 and np.abs(r0["pred"] - plain["pred"]).max() > 1e-3
    assert np.array_equal(VO.infer(cfg, shape, w, st, x), VO.infer(VO.CFG_A, shape, w, st, x))
