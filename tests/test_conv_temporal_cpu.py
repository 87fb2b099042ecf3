"""models.conv_temporal without a GPU: the oracle's 'same' max-pool against hand-written values, the chain's block order, SS5.json's variable
list (names, order, shapes), the simple_dense_stage activation rule, every configuration error (raised without a device), the refusals of
the stem operators (seld_stem_conv_*, seld_pool2d_*: the library loads without a device, and a call that got as far as a launch returns
SELD_ERR_HIP there, as in tests/test_module_ops_cpu.py) and the Dropout streams of SS5's stages.  The model is planned on torch's `meta`
device (modules.ConvTemporalNet(..., device='meta')): every layer is constructed, nothing is allocated or run."""
import copy
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import conv_temporal_oracle as CT
from conftest import ROOT
from seld_amd import _lib, models, modules

INVALID, UNSUPPORTED, HIP = -1, -2, -3
SS5 = json.load(open(os.path.join(ROOT, "tests", "golden", "SS5.json")))


# ---------------------------------------------------------------- 1. the oracle's pool
def _pool_by_hand(x, p, q):
    """x [H, W]: the maximum of the in-bounds elements of every window of TensorFlow 'SAME' (out = ceil(n / p), pad_before = (out p - n) // 2)"""
    H, W = x.shape
    Ho, Wo = -(-H // p), -(-W // q)
    hb, wb = (Ho * p - H) // 2, (Wo * q - W) // 2
    out = np.empty((Ho, Wo))
    for i in range(Ho):
        for j in range(Wo):
            rows = [r for r in range(i * p - hb, i * p - hb + p) if 0 <= r < H]
            cols = [c for c in range(j * q - wb, j * q - wb + q) if 0 <= c < W]
            out[i, j] = max(x[r, c] for r in rows for c in cols)
    return out


def test_oracle_pool_matches_hand_written_values():
    assert CT.same_pads(52, 5) == (11, 1, 2)      # 11 outputs, 1 row of padding in front and 2 behind
    assert CT.same_pads(15, 2) == (8, 0, 1)       # 8 outputs, none in front and 1 behind
    rng = np.random.default_rng(0)
    x = rng.standard_normal((52, 15)) - 3.0       # all windows' maxima negative: a zero padding would win
    y = CT.maxpool2d(torch.tensor(x)[None, :, :, None], (5, 2), "same")[0, :, :, 0].numpy()
    assert y.shape == (11, 8)
    assert np.array_equal(y, _pool_by_hand(x, 5, 2))
    # the first window holds rows 0 .. 3 only, the last one rows 49 .. 51; the last column window holds column 14 only
    assert y[0, 0] == x[0:4, 0:2].max() and y[10, 7] == x[49:52, 14:15].max() and y[1, 0] == x[4:9, 0:2].max()
    # torch's own symmetric padding of 1 would put row 0 .. 2 into the first window
    assert y[0, 0] != x[0:3, 0:2].max() or x[3, 0:2].max() < x[0:3, 0:2].max()
    w = CT.pool_windows(torch.tensor(x)[None, :, :, None], (5, 2), "same")
    assert tuple(w.shape) == (1, 11, 8, 10, 1) and np.array_equal(w.max(dim=3).values[0, :, :, 0].numpy(), y)
    assert bool(torch.isinf(w[0, 0, 0, :2, 0]).all()) and not bool(torch.isinf(w[0, 0, 0, 2:, 0]).any())
    yv = CT.maxpool2d(torch.tensor(x)[None, :, :, None], (5, 2), "valid")[0, :, :, 0].numpy()
    assert yv.shape == (10, 7) and yv[0, 0] == x[0:5, 0:2].max() and yv[9, 6] == x[45:50, 12:14].max()


# ---------------------------------------------------------------- 2. block order
def test_blocks_sort_as_strings():
    cfg = {"BLOCK2": "a", "BLOCK2_ARGS": {}, "BLOCK10": "b", "BLOCK10_ARGS": {}, "BLOCK0": "c", "BLOCK0_ARGS": {}, "SED": "x", "BLOCKS": "d"}
    assert modules.chain_blocks(cfg) == ["BLOCK0", "BLOCK10", "BLOCK2", "BLOCKS"] == CT.blocks_of(cfg)
    # in a model: BLOCK10 (3-D) in front of BLOCK2 (4-D) is the reference's order, and an error
    dense = {"units": [8]}
    bad = {"BLOCK2": "mother_block", "BLOCK2_ARGS": copy.deepcopy(CT.MOTHER), "BLOCK10": "simple_dense_block", "BLOCK10_ARGS": dense,
           "SED": "identity_block", "SED_ARGS": {}, "DOA": "identity_block", "DOA_ARGS": {}}
    with pytest.raises(ValueError, match="BLOCK2"):
        models.conv_temporal((1, 10, 8, 2), bad)
    good = {k.replace("BLOCK10", "BLOCK3"): v for k, v in bad.items()}
    m = modules.ConvTemporalNet((1, 10, 8, 2), good, "meta")
    assert [n for n, _, _ in m.variables if n.startswith("b")][0].startswith("b0.mb0.") and any(n.startswith("b1.dense0") for n, _, _ in m.variables)


# ---------------------------------------------------------------- 3. SS5.json's variables
def test_ss5_variable_names_order_and_shapes():
    shape = (4, 300, 64, 7)
    m = modules.ConvTemporalNet(shape, SS5, "meta")
    got = [(n, s) for n, _, s in m.variables]
    tr, nt = CT.variable_specs(SS5, shape)
    assert got == tr and [(n, s) for n, _, s in m.state_variables] == nt
    assert got[:4] == [("stem.conv.kernel", (7, 7, 7, 32)), ("stem.conv.bias", (32,)), ("stem.bn.gamma", (32,)), ("stem.bn.beta", (32,))]
    # creation order: stem conv, stem BN, the blocks, the SED block, sed_out, the DOA block, doa_out
    first = lambda p: next(i for i, (n, _) in enumerate(got) if n.startswith(p))
    order = [first(p) for p in ("stem.conv", "stem.bn", "b0.", "b1.", "b2.", "sed.", "sed_out", "doa.", "doa_out")]
    assert order == sorted(order) and got[-2:] == [("doa_out.kernel", (128, 36)), ("doa_out.bias", (36,))]
    assert dict(got)["sed_out.kernel"] == (192, 12) and m.S == 60 and m.n_classes == 12      # outputs [60, 12] / [60, 36]
    # pool (5, 2): 64 -> 32 bins; strides (1, 3): -> 11.  Each of the two mother blocks concatenates its (strided) input with its 96 new
    # channels (connect2 = [1, 0, 1] with filters2 = 0, reference modules.py:268-278): 32 -> 128 -> 224 channels, d_model = 11 * 224 -> 192
    assert m.blocks[-1].out_shape == (60, 11, 224)
    assert dict(got)["b1.dense0.kernel"] == (1, 11 * 224, 192) and m.body[1].blocks[0].D == 192
    assert len({n for n, _ in got}) == len(got)
    assert [n for n, _ in nt][:2] == ["stem.bn.moving_mean", "stem.bn.moving_variance"]
    assert [n for n, _ in nt][-2:] == ["sed.cf0.bn.moving_mean", "sed.cf0.bn.moving_variance"]


# ---------------------------------------------------------------- 4. simple_dense_stage's activation
def test_simple_dense_stage_overwrites_dense_activation():
    """reference modules.py:101: dense_activation = model_config.get('activation', None) — SS5.json's "dense_activation": "relu" yields a
    LINEAR layer"""
    kind, a = modules.canonical_kind("simple_dense_stage", SS5["BLOCK1_ARGS"])
    assert kind == "simple_dense_block" and a["units"] == [192] and a["dense_activation"] is None
    assert SS5["BLOCK1_ARGS"]["dense_activation"] == "relu"      # the configuration itself is left alone
    m = modules.ConvTemporalNet((1, 300, 64, 7), SS5, "meta")
    assert isinstance(m.body[0], modules.DenseBlock) and m.body[0].act == modules.ACT[None] == 0
    cfg = copy.deepcopy(SS5)
    cfg["BLOCK1_ARGS"]["activation"] = "relu"
    assert modules.ConvTemporalNet((1, 300, 64, 7), cfg, "meta").body[0].act == modules.ACT["relu"]
    # the oracle restates the same rule on its own
    assert CT._wrap("simple_dense_stage", SS5["BLOCK1_ARGS"])[1]["dense_activation"] is None
    assert modules.canonical_kind("bidirectional_GRU_stage", {"depth": 2, "units": 128}) == ("bidirectional_GRU_block", {"depth": 2, "units": [128, 128]})
    assert modules.canonical_kind("identity_block", {})[1]["units"] == []


# ---------------------------------------------------------------- 5. configuration errors, without a device
def _small(**over):
    cfg = {"filters": 4, "first_kernel_size": 3, "first_pool_size": [2, 2], "n_classes": 3,
           "BLOCK0": "simple_dense_block", "BLOCK0_ARGS": {"units": [8]},
           "SED": "identity_block", "SED_ARGS": {}, "DOA": "identity_block", "DOA_ARGS": {}}
    cfg.update(over)
    return cfg


@pytest.mark.parametrize("over,match", [
    (dict(BLOCK1="mother_block", BLOCK1_ARGS=copy.deepcopy(CT.MOTHER)), "4-D"),                 # a 4-D kind behind a 3-D one
    (dict(BLOCK1="mother_stage", BLOCK1_ARGS=dict(CT.MOTHER, depth=1)), "4-D"),
    (dict(BLOCK1="no_such_block", BLOCK1_ARGS={}), "no_such_block"),                             # an unknown kind
    (dict(BLOCK1="simple_conv_block", BLOCK1_ARGS={}), "simple_conv_block"),                     # a kind of the fused models
    (dict(SED="mother_block", SED_ARGS=copy.deepcopy(CT.MOTHER)), "SED"),                        # a 4-D kind as a head
    (dict(DOA="nothing"), "DOA"),
    (dict(BLOCK0="identity_block", BLOCK0_ARGS={}, BLOCK1="mother_block", BLOCK1_ARGS=copy.deepcopy(CT.MOTHER)), "4-D"),
    (dict(BLOCK0_ARGS={"units": [8], "dropout_rate": 0.2}), "dropout_rate must be 0"),           # the dense block's Dropout
    (dict(BLOCK0_ARGS={"units": [8], "dense_activation": "gelu"}), "dense_activation"),
    (dict(BLOCK1="bidirectional_GRU_stage", BLOCK1_ARGS={"depth": 1, "units": 64}), "128 units"),
    (dict(BLOCK1="conformer_encoder_stage", BLOCK1_ARGS={"depth": 1, "key_dim": 12}), "key_dim"),
    (dict(first_pool_size=[16, 16]), "255"),                                                       # the pooling position is a uint8
])
def test_configuration_errors_need_no_device(over, match):
    cfg = _small(**over)
    with pytest.raises(ValueError, match=match):
        models.conv_temporal((2, 20, 8, 3), cfg)


def test_identity_head_on_a_4d_tensor_and_missing_args():
    cfg = _small()
    del cfg["BLOCK0"], cfg["BLOCK0_ARGS"]
    with pytest.raises(ValueError, match="identity_block on a 4-D tensor"):      # the reference's Dense would emit a 4-D output
        models.conv_temporal((2, 20, 8, 3), cfg)
    cfg["SED"], cfg["SED_ARGS"] = "simple_dense_block", {"units": [5]}           # any other 3-D head flattens it
    cfg["DOA"], cfg["DOA_ARGS"] = "simple_dense_stage", {"depth": 1, "units": 5}
    m = modules.ConvTemporalNet((2, 20, 8, 3), cfg, "meta")
    assert dict((n, s) for n, _, s in m.variables)["sed.dense0.kernel"] == (1, 4 * 4, 5) and m.S == 10
    cfg = _small()
    del cfg["BLOCK0_ARGS"]
    with pytest.raises(ValueError, match="BLOCK0_ARGS"):
        models.conv_temporal((2, 20, 8, 3), cfg)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP device"):      # a valid configuration gets as far as the device
            models.conv_temporal((2, 20, 8, 3), _small())


def test_outside_the_stem_kernels_contract_is_im2col_not_an_error():
    for k, ch, direct in ((7, 7, True), (4, 7, False), (7, 17, False), (9, 3, False), (1, 16, True)):
        m = modules.ConvTemporalNet((1, 20, 8, ch), _small(first_kernel_size=k), "meta")
        assert (m.stem_conv.direct_fwd, m.stem_conv.direct_wgrad) == (direct and modules.StemConv2D.DIRECT["fwd"], direct and modules.StemConv2D.DIRECT["wgrad"])
        assert dict((n, s) for n, _, s in m.variables)["stem.conv.kernel"] == (k, k, ch, 4)


# ---------------------------------------------------------------- 6. the operators' refusals
OPS = {
    "seld_stem_conv_fwd": [("x", "p"), ("kernel", "p"), ("bias", "p"), ("z", "p"), ("B", 1), ("H", 4), ("W", 4), ("Cin", 2), ("k", 3), ("F", 4)],
    "seld_stem_conv_wgrad": [("x", "p"), ("dz", "p"), ("dkernel", "p"), ("dbias", "p"), ("scratch", "p"), ("B", 1), ("H", 4), ("W", 4), ("Cin", 2),
                             ("k", 3), ("F", 4)],
    "seld_pool2d_fwd": [("x", "p"), ("y", "p"), ("idx", "o"), ("B", 1), ("H", 4), ("W", 4), ("C", 4), ("ph", 2), ("pw", 2), ("same", 1, "v")],
    "seld_pool2d_bwd": [("dy", "p"), ("idx", "p"), ("dx", "p"), ("B", 1), ("H", 4), ("W", 4), ("C", 4), ("ph", 2), ("pw", 2), ("same", 1, "v")],
}


@pytest.fixture(scope="module")
def env(seld_lib):
    gpu = torch.cuda.is_available()
    buf = torch.zeros(1 << 16, device="cuda") if gpu else None
    yield seld_lib, (C.c_void_p(buf.data_ptr()) if gpu else C.c_void_p(1 << 20)), gpu      # no device: never dereferenced, a launch fails first
    del buf


def _call(env, op, **over):
    lib, p, _ = env
    args = []
    for spec in OPS[op]:
        name, val = spec[0], spec[1]
        args.append(over[name] if name in over else (p if val in ("p", "o") else val))
    return getattr(lib, op)(*args, None)


@pytest.mark.parametrize("op", sorted(OPS))
def test_operator_base_call_is_valid(env, op):
    assert _call(env, op) == (0 if env[2] else HIP)
    if env[2]:
        torch.cuda.synchronize()


def _bad_cases():
    for op, spec in OPS.items():
        for s in spec:
            if s[1] == "p":
                yield op, {s[0]: None}
            elif s[1] != "o" and len(s) == 2:
                yield op, {s[0]: 0}
                yield op, {s[0]: -1}


@pytest.mark.parametrize("op,bad", list(_bad_cases()), ids=lambda v: v if isinstance(v, str) else ",".join(f"{k}={v[k]}" for k in v))
def test_operator_refuses_null_pointer_and_size_below_one(env, op, bad):
    assert _call(env, op, **bad) == INVALID


def test_operator_refuses_what_the_header_documents(env):
    lib = env[0]
    for op in ("seld_stem_conv_fwd", "seld_stem_conv_wgrad"):
        for k in (2, 4, 6, 8, 9):
            assert _call(env, op, k=k) == UNSUPPORTED
        assert _call(env, op, Cin=17) == UNSUPPORTED
        assert _call(env, op, Cin=16, k=7, H=1, W=1) == (0 if env[2] else HIP)      # the corners of the contract are inside it
        assert _call(env, op, k=2, B=0) == INVALID                                   # a size below one comes first
    assert lib.seld_stem_conv_wgrad_scratch(1, 4, 4, 2, 2, 4) == UNSUPPORTED and lib.seld_stem_conv_wgrad_scratch(1, 4, 4, 17, 3, 4) == UNSUPPORTED
    assert lib.seld_stem_conv_wgrad_scratch(0, 4, 4, 2, 3, 4) == INVALID
    # one 8 x 32 tile -> one partial of [k k Cin + 1][F]; never more than 512 partials
    assert lib.seld_stem_conv_wgrad_scratch(1, 4, 4, 2, 3, 4) == (3 * 3 * 2 + 1) * 4
    assert lib.seld_stem_conv_wgrad_scratch(2, 9, 33, 7, 7, 32) == 2 * 2 * 2 * (49 * 7 + 1) * 32
    assert lib.seld_stem_conv_wgrad_scratch(32, 300, 64, 7, 7, 32) == 512 * (49 * 7 + 1) * 32
    for op in ("seld_pool2d_fwd", "seld_pool2d_bwd"):
        assert _call(env, op, H=16, W=16, ph=16, pw=16) == UNSUPPORTED      # ph * pw = 256: the position is a uint8
        assert _call(env, op, H=16, W=17, ph=15, pw=17) == (0 if env[2] else HIP)      # 255 fits
        assert _call(env, op, ph=5, pw=2, same=0) == INVALID                 # 'valid' with a pool larger than the tensor: an empty output
        assert _call(env, op, ph=5, pw=2, same=1) == (0 if env[2] else HIP)
    assert _call(env, "seld_pool2d_fwd", idx=None) == (0 if env[2] else HIP)      # inference: no positions
    if env[2]:
        torch.cuda.synchronize()


# ---------------------------------------------------------------- 7. Dropout streams
def test_ss5_stages_draw_from_distinct_streams():
    m = modules.ConvTemporalNet((1, 300, 64, 7), SS5, "meta")
    # blocks built in front of each stage: 2 mother blocks + 1 dense block; + 2 conformer blocks; + 1 conformer block
    D0 = modules.DROP_STREAM0
    assert m.stream_bases == {"b2.cf": D0 + 32 * 3, "sed.cf": D0 + 32 * 5, "doa.gru": D0 + 32 * 6}
    bases = [blk.drop.base for st in (m.body[1], m.heads[0].body) for blk in st.blocks]
    assert bases == [D0 + 96, D0 + 128, D0 + 160] and len(set(bases)) == 3
    # seven sites per conformer block: no two blocks' streams overlap
    assert all(b2 - b1 >= 7 for b1, b2 in zip(bases, bases[1:]))
    assert all(blk.drop.rate == pytest.approx(0.1) for st in (m.body[1], m.heads[0].body) for blk in st.blocks)      # SS5.json names no rate
    # models.seldnet's numbering is what it was: a stage built alone starts at DROP_STREAM0
    rt = modules._Rt(torch.device("meta"))
    rt.dropout = True
    st = modules._build_second("conformer_encoder_stage", rt, SS5["BLOCK2_ARGS"], 60, 192, 1)
    assert [b.drop.base for b in st.blocks] == [D0, D0 + 32]
