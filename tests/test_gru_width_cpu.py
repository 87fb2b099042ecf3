"""The any-width GRU (seld_rnn_gruw_*, modules' any_units, ConvTemporalNet search=True) and the SELD architecture search (seld_amd/nas_seldnet.py)
without a device: what seld_rnn_gruw_plan reports and the case lists tests/test_gru_width_gpu.py derives from it, the fp32 margin of every one
of those cases (the rule of tests/test_rnn_cpu.py), the entries' refusal order (the library loads without a device; a call that got as far
as a launch returns SELD_ERR_HIP there, so the code shows that the refusal came first — tests/test_module_ops_cpu.py), the configuration
rules, the plan against the oracle's variable list, and the search: spaces, sampler, constraint, main's resume check."""
import copy
import ctypes as C
import json

import numpy as np
import pytest
import torch

import conv_temporal_oracle as CT
import gru_width_cases as G
from helpers import rel_err

INVALID, UNSUPPORTED, HIP = -1, -2, -3


# ---------------------------------------------------------------- the plan and the case lists
def test_plan_is_valid_for_every_width_and_refuses_the_rest(seld_lib):
    out = (C.c_int32 * 4)()
    n_forms = {seld_lib.seld_rnn_gruw_plan(u, out) for u in range(1, G.MAX_UNITS + 1)}
    assert len(n_forms) == 1 and min(n_forms) >= 1
    for u in range(1, G.MAX_UNITS + 1):
        (form, tile, fc, bc), n = G.gruw_plan(u)
        assert 0 <= form < n and tile >= 1 and fc >= 1 and bc >= 1, (u, form, tile, fc, bc)
    for u in (0, G.MAX_UNITS + 1, -1):
        assert seld_lib.seld_rnn_gruw_plan(u, out) == UNSUPPORTED


def test_case_lists_bracket_what_the_plan_reports():
    ws = G.widths()
    assert set(G.SEARCH_UNITS) <= set(ws) and {1, 3, 100, 127, 129, 255} <= set(ws)
    for u in range(2, G.MAX_UNITS + 1):
        if G.gruw_plan(u)[0][:2] != G.gruw_plan(u - 1)[0][:2]:
            assert u - 1 in ws and u in ws
    assert {G.gruw_plan(u)[0][0] for u in ws} == set(range(G.gruw_plan(1)[1])), "a form no width of the list reaches"
    for u in ws:
        (_, t, fc, bc), _ = G.gruw_plan(u)
        s, b = set(G.s_values(u)), set(G.b_values(u))
        assert {1, 2, 60} <= s and all(v in s for c in (fc, bc) for v in (c - 1, c, c + 1, 2 * c + 1) if v >= 1)
        assert 1 in b and ({t - 1, t, t + 1} <= b if t > 1 else {1, 3} <= b)
        assert len(G.cases(u)) == len(s) * len(b)
    assert set(G.one_width_per_form()) == set(range(G.gruw_plan(1)[1]))


@pytest.mark.parametrize("u", G.widths())
def test_fp32_margin_of_the_kernel_cases(u):
    """h, the saved gates, dgx and dgh (per direction, per gate third, per plane) of a plain fp32 evaluation against fp64"""
    for B, S in G.cases(u):
        _, r64 = G.reference(B, S, u)
        _, r32 = G.reference(B, S, u, fp32=True)
        G.compare(f"u{u} {(B, S)}", G.as_kernel_outputs(r32), r64, u, G.FP32_MARGIN)


def test_fp32_margin_of_the_saturated_and_128_cases():
    B, S, scale = G.SATURATED
    for u in list(G.one_width_per_form().values()) + [128]:
        _, r64 = G.reference(B, S, u, scale if u != 128 else 1.0)
        _, r32 = G.reference(B, S, u, scale if u != 128 else 1.0, fp32=True)
        G.compare(f"u{u} x{scale}", G.as_kernel_outputs(r32), r64, u, G.FP32_MARGIN)


def test_fp32_margin_of_the_block_and_model_cases():
    import rnn_oracle as R
    for name, (_, B, S, D, depth, cfg) in G.BLOCK_CASES.items():
        a, b = R.stage_reference(B, S, D, depth, cfg, 3, torch.float32), R.stage_reference(B, S, D, depth, cfg, 3)
        for k in ("out", "dx", "grad"):
            assert rel_err(a[k], b[k]) <= G.FP32_MARGIN, (name, k)
    B, S, D, cfg = G.GRU_BLOCK_CASE
    a, b = G.gru_block_reference(B, S, D, cfg, 3, torch.float32), G.gru_block_reference(B, S, D, cfg, 3)
    for k in ("out", "dx", "grad"):
        assert rel_err(a[k], b[k]) <= G.FP32_MARGIN, k
    for name in G.MODELS:
        cfg, shape, w, st, x, ys, yd, ref = G.model_reference(name)
        r32 = CT.train_step(cfg, shape, w, st, x, ys, yd, doa_loss="MSE", loss_weight=(1.0, 1000.0), lr=1e-3, step=1, dtype=torch.float32)
        for k in ("sed", "doa", "grad"):
            assert rel_err(r32[k], ref[k]) <= G.FP32_MARGIN, (name, k)


# ---------------------------------------------------------------- refusal order, without a device
FWD = ["gx_f", "gx_b", "U_f", "U_b", "brec_f", "brec_b", "h_f", "h_b", "saved_f", "saved_b"]
BWD = ["dh_f", "dh_b", "h_f", "h_b", "saved_f", "saved_b", "U_f", "U_b", "dgx_f", "dgx_b", "dgh_f", "dgh_b"]
OPTIONAL = {"saved_f", "saved_b"}      # of the forward: NULL at inference


@pytest.fixture(scope="module")
def env(seld_lib):
    gpu = torch.cuda.is_available()
    buf = torch.zeros(1 << 18, device="cuda") if gpu else None      # U [256, 768] is the largest operand of the base call
    p = C.c_void_p(buf.data_ptr()) if gpu else C.c_void_p(1 << 20)     # no device: never dereferenced, a launch fails first
    yield seld_lib, p, gpu
    del buf


def _call(env, op, names, B=1, S=1, units=5, **over):
    lib, p, _ = env
    args = [over.get(n, p) for n in names]
    return getattr(lib, op)(*args, B, S, units, None)


@pytest.mark.parametrize("op,names", [("seld_rnn_gruw_fwd", FWD), ("seld_rnn_gruw_bwd", BWD)])
def test_refusal_order_of_the_entries(env, op, names):
    assert _call(env, op, names) == (0 if env[2] else HIP), "the base call must get as far as its launch"
    one = {n: None for n in names if n.endswith("_b")}
    assert _call(env, op, names, **one) == (0 if env[2] else HIP), "one direction is a valid call"
    if env[2]:
        torch.cuda.synchronize()
    for u in (0, G.MAX_UNITS + 1, -3):
        assert _call(env, op, names, units=u, B=0) == UNSUPPORTED      # the width first, whatever else is wrong
        assert _call(env, op, names, units=u, **{names[0]: None}) == UNSUPPORTED
    for n in names:
        if n.endswith("_f") and not (op.endswith("fwd") and n in OPTIONAL):
            assert _call(env, op, names, **{n: None}) == INVALID, n
    for bad in ({"B": 0}, {"B": -1}, {"S": 0}, {"S": -1}):
        assert _call(env, op, names, **bad) == INVALID, bad
    for n in names:      # half a direction: one *_b argument missing, and one *_b argument alone
        if n.endswith("_b"):
            assert _call(env, op, names, **{n: None}) == INVALID, n
            if n != names[1]:      # names[1] (gx_b / dh_b) decides how many directions there are
                assert _call(env, op, names, **{m: None for m in one if m != n}) == INVALID, n
    if op.endswith("fwd"):      # saved for one direction only
        assert _call(env, op, names, saved_f=None) == INVALID
    assert _call(env, op, names, B=1 << 30, S=1 << 30) == UNSUPPORTED      # beyond the 64-bit offsets' stated bound
    assert _call(env, op, names, B=(1 << 30) + 1) == UNSUPPORTED


# ---------------------------------------------------------------- configuration rules
def test_any_units_config_rules():
    from seld_amd.modules import check_gru_config, check_rnn_config
    for u in (1, 5, 64, 256):
        check_rnn_config({"units": u}, any_units=True)
        check_rnn_config({"units": u, "depth": 2, "merge_mode": "concat"}, True, any_units=True)
        check_gru_config({"units": [u]}, any_units=True)
    check_gru_config({"units": [192, 128, 4]}, any_units=True)
    for u in (0, 257, 12.5, "12", [12], None, True):
        with pytest.raises(ValueError, match="1..256"):
            check_rnn_config({"units": u}, any_units=True)
        with pytest.raises(ValueError, match="1..256"):
            check_gru_config({"units": [128, u]}, any_units=True)
    for kw in ({}, {"any_units": True}):      # the LSTM kernels are not part of this
        with pytest.raises(ValueError, match="128 units"):
            check_rnn_config({"units": 64, "rnn_type": "LSTM"}, **kw)
        check_rnn_config({"units": 128, "rnn_type": "LSTM"}, **kw)
    with pytest.raises(ValueError, match="DROP forms"):
        check_rnn_config({"units": 64, "dropout_rate": 0.2}, dropout=True, any_units=True)
    with pytest.raises(ValueError, match="DROP forms"):
        check_gru_config({"units": [128, 64], "dropout_rate": 0.2}, dropout=True, any_units=True)
    check_rnn_config({"units": 128, "dropout_rate": 0.2}, dropout=True, any_units=True)
    check_gru_config({"units": [128, 128], "dropout_rate": 0.2}, dropout=True, any_units=True)
    # without the keyword: today's refusals, in today's words
    with pytest.raises(ValueError, match="units 64: the recurrence kernels are built for 128 units"):
        check_rnn_config({"units": 64})
    with pytest.raises(ValueError, match="^the recurrence kernels are built for 128 units$"):
        check_gru_config({"units": [128, 64]})


@pytest.mark.parametrize("name", sorted(G.MODELS))
def test_plan_equals_oracle(name):
    from seld_amd import models
    from seld_amd.modules import ConvTemporalNet
    cfg, shape = G.MODELS[name]
    tr, nt = CT.variable_specs(cfg, shape)
    m = ConvTemporalNet(shape, cfg, "meta", search=True)
    assert [(n, s) for n, _, s in m.variables] == tr and [(n, s) for n, _, s in m.state_variables] == nt
    cx = m.complexity()
    assert cx["params"] == sum(int(np.prod(s)) for _, s in tr) and cx["flops"] > 0
    for build in (lambda: ConvTemporalNet(shape, cfg, "meta"), lambda: ConvTemporalNet(shape, cfg, "meta", search=False),
                  lambda: models.conv_temporal(shape, cfg, "meta")):
        with pytest.raises(ValueError, match="128 units"):
            build()


def test_complexity_counts_the_recurrent_products():
    from seld_amd.modules import ConvTemporalNet
    cfg = copy.deepcopy(G.CONFIG_A)
    base = ConvTemporalNet(G.INPUT_A, cfg, "meta", search=True).complexity()
    cfg["SED_ARGS"]["units"] = 7      # SED: D = 12 -> GRU(7) both directions -> Dense(3)
    wide = ConvTemporalNet(G.INPUT_A, cfg, "meta", search=True).complexity()
    S, D, nc = 9, 12, 3
    per = lambda u: 2 * S * (D + u) * 3 * u + S * u * nc
    assert wide["flops"] - base["flops"] == per(7) - per(5)


# ---------------------------------------------------------------- the search
def test_search_spaces_hold_the_reference_values():
    from seld_amd import nas_seldnet as N
    units = [4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256]
    filters = [0] * 11 + [3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256]
    assert N.search_space_1d == {"bidirectional_GRU_stage": {"depth": [1, 2, 3], "units": units},
                                 "simple_dense_stage": {"depth": [1, 2, 3], "units": units, "dense_activation": ["relu"],
                                                        "dropout_rate": [0., 0.2, 0.5]}}
    assert list(N.search_space_2d) == ["mother_stage"]
    ms = N.search_space_2d["mother_stage"]
    assert ms["depth"] == [1, 2, 3] and all(ms[f"filters{i}"] == filters and ms[f"kernel_size{i}"] == [1, 3, 5] for i in range(3))
    assert ms["connect0"] == [[0], [1]] and ms["connect1"] == [[0, 0], [0, 1], [1, 0], [1, 1]] and len(ms["connect2"]) == 8
    assert ms["connect2"][3] == [0, 1, 1] and ms["strides"] == [(1, 1), (1, 2), (1, 3)]
    N.search_space_sanity_check(N.search_space_2d), N.search_space_sanity_check(N.search_space_1d)
    from seld_amd import nas_vad
    assert N.search_space_sanity_check is nas_vad.search_space_sanity_check and N.postprocess_fn is nas_vad.postprocess_fn


def test_sampler_draws_blocks_and_both_heads_and_is_seeded():
    from seld_amd import nas_seldnet as N
    draw = lambda seed: N.conv_temporal_sampler(N.search_space_2d, N.search_space_1d, 4, [300, 64, 7], {"n_classes": 12}, N.postprocess_fn,
                                                None, np.random.default_rng(seed))
    for seed in range(8):
        c = draw(seed)
        assert sorted(k for k in c if not k.endswith("_ARGS")) == ["BLOCK0", "BLOCK1", "BLOCK2", "BLOCK3", "DOA", "SED", "n_classes"]
        seen_1d = False
        for i in range(4):      # 2-D blocks first, then 1-D ones
            one_d = c[f"BLOCK{i}"] in N.search_space_1d
            assert one_d or (c[f"BLOCK{i}"] in N.search_space_2d and not seen_1d)
            seen_1d |= one_d
        for head in ("SED", "DOA"):
            space = N.search_space_1d[c[head]]
            assert set(c[f"{head}_ARGS"]) == set(space) and all(c[f"{head}_ARGS"][k] in space[k] for k in space)
        assert c == draw(seed)
    assert any(draw(s) != draw(0) for s in range(1, 8))
    with pytest.raises(RuntimeError, match="no configuration"):
        N.conv_temporal_sampler(N.search_space_2d, N.search_space_1d, 2, [300, 64, 7], None, None, lambda c, s: False, np.random.default_rng(0), 5)


def _space_cases():
    from seld_amd import nas_seldnet as N
    for kind, space in N.search_space_1d.items():
        for arg, values in space.items():
            for v in values:
                yield kind, arg, v


@pytest.mark.parametrize("kind,arg,value", list(_space_cases()), ids=lambda v: str(v))
def test_constraint_accepts_every_value_of_the_1d_space(kind, arg, value):
    """as BLOCK0 and as both heads, on the meta device: the whole 1-D space can be built (12 of the 13 GRU widths and two of the three
    dropout rates could not, before seld_rnn_gruw_* and search=True)"""
    from seld_amd import nas_seldnet as N
    args = {k: v[0] for k, v in N.search_space_1d[kind].items()}
    args[arg] = value
    cfg = {"n_classes": 12, "BLOCK0": kind, "BLOCK0_ARGS": dict(args), "SED": kind, "SED_ARGS": dict(args), "DOA": kind, "DOA_ARGS": dict(args)}
    assert N.sample_constraint()(N.postprocess_fn(cfg), [2, 300, 64, 7])


def test_constraint_rejects_degenerate_mother_stages_and_an_empty_window():
    from seld_amd import nas_seldnet as N
    head = {"depth": 1, "units": 8}
    ms = dict(CT.MOTHER, depth=1, filters1=6, strides=[1, 2])
    mk = lambda **kw: N.postprocess_fn({"n_classes": 12, "BLOCK0": "mother_stage", "BLOCK0_ARGS": dict(ms, **kw),
                                        "SED": "bidirectional_GRU_stage", "SED_ARGS": dict(head), "DOA": "bidirectional_GRU_stage",
                                        "DOA_ARGS": dict(head)})
    ok = N.sample_constraint()
    shape = [2, 300, 64, 7]
    assert ok(mk(), shape)
    assert not ok(mk(filters0=8, filters1=0, kernel_size0=3), shape)      # one convolution that is not the strided one
    assert not ok(mk(filters0=8, kernel_size0=3, strides=[1, 1]), shape)      # two convolutions, the second without strides
    cx = N.plan(mk(), shape).complexity()
    assert not N.sample_constraint(cx["flops"] + 1, None)(mk(), shape) and not N.sample_constraint(None, cx["flops"] - 1)(mk(), shape)
    assert not N.sample_constraint(None, None, cx["params"] + 1, None)(mk(), shape)
    assert N.sample_constraint(cx["flops"], cx["flops"], cx["params"], cx["params"])(mk(), shape)
    bad = mk()
    bad["SED_ARGS"]["units"] = 300      # what the plan refuses with a ValueError is rejected, not raised
    assert not ok(bad, shape)


def test_main_refuses_another_train_config_without_a_device(tmp_path):
    from seld_amd import nas_seldnet as N
    name = str(tmp_path / "run.json")
    argv = ["--name", name, "--dataset_path", str(tmp_path / "nowhere"), "--n_samples", "2"]
    prev = {"train_config": dict(vars(N.get_parser().parse_args(argv)), lr=0.5)}
    with open(name, "w") as f:
        json.dump(prev, f)
    with pytest.raises(ValueError, match="different train_config"):
        N.main(argv)
