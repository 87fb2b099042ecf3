"""xception_block's per-kernel entry points (seld_k_xc_*, include/seld_hip.h) and their reference (tests/xception_oracle.py), checked without a
GPU.  Refusals as in tests/test_module_ops_cpu.py: each call is one valid call with ONE argument made bad; the library loads without a device, where
a call that got as far as its scratch allocation or a launch returns SELD_ERR_NOMEM or SELD_ERR_HIP, so the return code shows that the refusal
came first.  The reference itself is tied to oracle/seldnet_oracle.py: its units chained over one module must be the spec's middle flow."""
import ctypes as C

import numpy as np
import pytest
import torch

import xception_oracle as X

INVALID, UNSUPPORTED, HIP, NOMEM = -1, -2, -3, -4

# one valid call per entry point: (argument name, kind, value).  kinds: p required pointer, o pointer that may be NULL, s size (refused at 0 and -1),
# v anything else.  The sizes keep every buffer within BUF_FLOATS.
OPS = {
    "seld_k_xc_dw_fwd": [("x", "p", 0), ("k", "p", 0), ("aff", "o", 0), ("y", "p", 0), ("B", "s", 1), ("H", "s", 2), ("W", "s", 16)],
    "seld_k_xc_unit_fwd": [("x", "p", 0), ("kdw", "p", 0), ("wpw", "p", 0), ("aff", "o", 0), ("dwo", "p", 0), ("z", "p", 0), ("sums", "o", 0),
                           ("B", "s", 1), ("H", "s", 2), ("fused", "v", 1)],
    "seld_k_xc_pw_bwd": [("z", "p", 0), ("gy", "p", 0), ("dwo", "p", 0), ("wpw", "p", 0), ("mean", "p", 0), ("invstd", "p", 0), ("scale", "p", 0),
                         ("c1c2", "p", 0), ("f1", "p", 0), ("dw", "p", 0), ("npix", "s", 33), ("mode", "v", 1)],
    "seld_k_xc_bn_stats": [("z", "p", 0), ("sums", "p", 0), ("npix", "s", 33)],
    "seld_k_xc_bn_apply": [("z", "p", 0), ("scale", "p", 0), ("shift", "p", 0), ("res", "o", 0), ("out", "p", 0), ("npix", "s", 33)],
    "seld_k_xc_bn_bwd": [("z", "p", 0), ("dy", "p", 0), ("mean", "p", 0), ("invstd", "p", 0), ("scale", "p", 0), ("dz", "p", 0), ("dgamma", "p", 0),
                         ("dbeta", "p", 0), ("c1c2", "p", 0), ("npix", "s", 33)],
}
BUF_FLOATS = 1 << 14      # the largest base call: 33 pixels x 64 channels; the pointwise weights [64][64]


@pytest.fixture(scope="module")
def env(seld_lib):
    """(library, pointer for every buffer, whether a device is present)"""
    gpu = torch.cuda.is_available()
    buf = torch.zeros(BUF_FLOATS, device="cuda") if gpu else None
    p = C.c_void_p(buf.data_ptr()) if gpu else C.c_void_p(1 << 20)     # no device: never dereferenced, a launch fails first
    yield seld_lib, p, gpu
    del buf


def _call(env, op, **over):
    lib, p, _ = env
    args = []
    for name, kind, val in OPS[op]:
        v = over.get(name, val)
        if kind in "po" and name not in over:
            v = p
        args.append(v)
    return getattr(lib, op)(*args)


def _got_through(env, rc):
    """past every refusal: SELD_OK with a device; without one the scratch allocation (SELD_ERR_NOMEM) or the launch (SELD_ERR_HIP) fails"""
    return rc == 0 if env[2] else rc in (HIP, NOMEM)


def _cases():
    for op, spec in OPS.items():
        for name, kind, _ in spec:
            if kind == "p":
                yield op, {name: None}
            elif kind == "s":
                yield op, {name: 0}
                yield op, {name: -1}


@pytest.mark.parametrize("op", sorted(OPS))
def test_base_call_is_valid(env, op):
    """The unmodified call gets as far as its allocations and launches — SELD_OK on the placeholder buffer with a device — so the refusals
    below are the bad argument's.  So does the call with every optional pointer NULL."""
    assert _got_through(env, _call(env, op))
    assert _got_through(env, _call(env, op, **{n: None for n, kind, _ in OPS[op] if kind == "o"}))
    if env[2]:
        torch.cuda.synchronize()


@pytest.mark.parametrize("op,bad", list(_cases()), ids=lambda v: v if isinstance(v, str) else ",".join(f"{k}={v[k]}" for k in v))
def test_refuses_null_pointer_and_size_below_one(env, op, bad):
    assert _call(env, op, **bad) == INVALID


def test_every_route_is_reached_and_refuses_alike(env):
    """the unfused forward, the three pointwise-backward modes: each a valid call; the fused forward writes dwo and z whatever else is asked of
    it, so neither may be missing in either form; an unknown mode is refused"""
    for fused in (0, 1):
        for sums in ({}, {"sums": None}):
            assert _got_through(env, _call(env, "seld_k_xc_unit_fwd", fused=fused, **sums))
            assert _call(env, "seld_k_xc_unit_fwd", fused=fused, dwo=None, **sums) == INVALID
            assert _call(env, "seld_k_xc_unit_fwd", fused=fused, z=None, **sums) == INVALID
    for mode in (0, 1, 2):
        assert _got_through(env, _call(env, "seld_k_xc_pw_bwd", mode=mode))
        assert _call(env, "seld_k_xc_pw_bwd", mode=mode, f1=None) == INVALID
        assert _call(env, "seld_k_xc_pw_bwd", mode=mode, npix=0) == INVALID
    for mode in (-1, 3):
        assert _call(env, "seld_k_xc_pw_bwd", mode=mode) == INVALID
    if env[2]:
        torch.cuda.synchronize()


def test_refuses_sizes_the_launchers_index_cannot_hold(env):
    """row, tile and product-row counts are ints in the launchers: UNSUPPORTED before anything is enqueued"""
    assert _call(env, "seld_k_xc_dw_fwd", B=1 << 15, H=1 << 15, W=16) == UNSUPPORTED
    assert _call(env, "seld_k_xc_unit_fwd", B=1 << 14, H=1 << 14) == UNSUPPORTED
    assert _call(env, "seld_k_xc_unit_fwd", B=1 << 14, H=1 << 14, fused=0) == UNSUPPORTED
    assert _call(env, "seld_k_xc_pw_bwd", npix=1 << 31, mode=0) == UNSUPPORTED
    assert _call(env, "seld_k_xc_bn_apply", npix=(1 << 35) + 1) == UNSUPPORTED
    assert _call(env, "seld_k_xc_bn_bwd", npix=(1 << 35) + 1) == UNSUPPORTED


def test_reference_units_chain_to_the_specs_middle_flow(xception_config):
    """xception_oracle's unit_forward + BatchNormalization over one module of three units plus the residual = oracle/seldnet_oracle.py's middle
    flow for the same weights, in float64"""
    import copy
    from oracle import seldnet_oracle as O
    cfg = copy.deepcopy(xception_config)
    cfg["FIRST_ARGS"]["block_num"] = 1
    spec = O.Spec.from_config(cfg)
    w, st = O.random_weights(spec, 3)
    x, ys, yd = O.synthetic_batch(2, 15)
    taps = O.train_step(spec, w, st, x, ys, yd, dtype=torch.float64, want_taps=True)["taps"]
    named = O.unflatten(torch.as_tensor(np.asarray(w)).to(torch.float64), O.variable_specs(spec)[0])
    units = [(named[f"xc0.{u}.depthwise_kernel"][:, :, :, 0], named[f"xc0.{u}.pointwise_kernel"][0, 0], named[f"xc0.{u}.gamma"],
              named[f"xc0.{u}.beta"]) for u in range(3)]
    h = taps["pool0"]
    assert h.shape == (2, 3, 16, 64) and h.dtype == np.float64
    got = X.module_forward(h, units).numpy()
    err = np.abs(got - taps["xc0"]).max() / np.abs(taps["xc0"]).max()
    print(f"[oracle] module chain vs seldnet_oracle middle flow: rel err {err:.2e}")
    assert err <= 1e-12


def _all_gate_cases():
    for B, H, W in X.DW_FWD_W16 + X.DW_FWD_GENERIC:
        yield B, H, W
    for B, H in X.UNIT_SHAPES + [X.UNIT_BIG, X.DW_BWD_BIG]:
        yield B, H, 16


@pytest.mark.parametrize("B,H,W", sorted(set(_all_gate_cases())))
def test_gate_margin_helper_reaches_its_condition(B, H, W):
    """min |x scale + shift| >= 1e-4 (min |x| without aff) in float64 after the helper, at every shape of the shared lists; it moves only the
    offending elements, each by 0.01 / scale"""
    x, _, _, aff = X.unit_inputs(B, H, W)
    for a in (aff, None):
        x2, moved = X.apply_gate_margin(x, a)
        assert x2.dtype == np.float32 and x2.shape == x.shape
        assert X.gate_margin(x2, a) >= X.GATE_MARGIN
        changed = x2 != x
        assert changed.sum() == moved == (np.abs(X.pre_activation(x, a)) < X.GATE_MARGIN).sum()
        sc = np.abs(a[:64]) if a is not None else np.ones(64)
        assert (np.abs(x2.astype(np.float64) - x) <= 0.0101 / sc)[changed].all()
        assert np.array_equal(np.sign(X.pre_activation(x2, a))[changed], np.where(X.pre_activation(x, a) >= 0, 1.0, -1.0)[changed])
    if (B, H) == X.UNIT_BIG:
        assert moved > 0      # 6.6 M standard-normal elements: some lie within 1e-4 of zero
