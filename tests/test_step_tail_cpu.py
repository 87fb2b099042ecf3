"""loss_adam.hip's per-kernel entry points (seld_k_losses_strided .. seld_k_dropout4, include/seld_hip.h) and their reference
(tests/step_tail_oracle.py), checked without a GPU.  Refusals as in tests/test_xception_kernels_cpu.py: each call is one valid call with ONE
argument made bad; the library loads without a device, where a call that got as far as a launch returns SELD_ERR_HIP, so SELD_ERR_INVALID shows
that the refusal came first.  The reference is tied to oracle/seldnet_oracle.py and to its own identities, a plain float32 evaluation of it must
stay within half of every bar of tests/test_step_tail_gpu.py, and every kernel of the file must be named by a GPU test."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import step_tail_oracle as T
from conftest import ROOT
from helpers import rel_err
from oracle import seldnet_oracle as O

INVALID, HIP = -1, -3

# one valid call per entry point: (argument name, kind, value).  kinds: p required pointer, o pointer that may be NULL, c the loss configuration,
# h a host int64 array, s size (refused at 0 and -1), v anything else.  Every buffer of a base call lies within BUF_FLOATS.
OPS = {
    "seld_k_losses_strided": [("sed", "p", 0), ("doa", "p", 0), ("y_sed", "p", 0), ("y_doa", "p", 0), ("cfg", "c", 0), ("sloss", "p", 0),
                              ("dloss", "p", 0), ("dsed_pre", "o", 0), ("ld_sed", "v", 0), ("ddoa_pre", "o", 0), ("ld_doa", "v", 0),
                              ("scratch", "p", 0), ("B", "s", 1), ("S", "s", 2), ("nc", "s", 4), ("defer_finalize", "v", 0)],
    "seld_k_losses_finalize": [("cfg", "c", 0), ("sloss", "p", 0), ("dloss", "p", 0), ("scratch", "p", 0), ("B", "s", 1), ("S", "s", 2),
                               ("nc", "s", 4)],
    "seld_k_agc": [("theta", "p", 0), ("g", "p", 0), ("off", "v", 8), ("rank", "v", 2), ("shape", "h", (3, 8))],
    "seld_k_act_bwd": [("y", "p", 0), ("dy", "p", 0), ("n", "s", 8), ("act", "v", 1)],
    "seld_k_v1_couple_fwd": [("sed", "p", 0), ("doa1", "p", 0), ("out", "p", 0), ("out2", "o", 0), ("rows", "s", 2), ("nc", "s", 4)],
    "seld_k_v1_couple_bwd": [("sed", "p", 0), ("doa1", "p", 0), ("dsed_pre", "p", 0), ("ld_sed", "v", 4), ("ddoa_pre", "p", 0), ("ld_doa", "v", 12),
                             ("rows", "s", 2), ("nc", "s", 4)],
    "seld_k_time_expand": [("x", "p", 0), ("xe", "p", 0), ("B", "s", 1), ("S", "s", 2), ("C", "s", 4), ("ks", "s", 3)],
    "seld_k_time_fold": [("dxe", "p", 0), ("dx", "p", 0), ("B", "s", 1), ("S", "s", 2), ("C", "s", 4), ("ks", "s", 3), ("accumulate", "v", 0)],
    "seld_k_mask_rows": [("in", "p", 0), ("mask", "p", 0), ("out", "p", 0), ("rows", "s", 4), ("S", "s", 2), ("F", "s", 4), ("accumulate", "v", 0)],
    "seld_k_dropout4": [("in", "p", 0), ("out", "p", 0), ("n", "s", 8), ("rate", "v", 0.25), ("seed", "v", 5), ("layer", "v", 1), ("step", "v", 2)],
}
BUF_FLOATS = 1 << 12
FILL = 7.0
# what each launcher refuses besides NULL and sizes below 1, and what the entry points add for the launchers' sake
BAD = [("seld_k_losses_strided", {"ld_sed": 3}), ("seld_k_losses_strided", {"ld_doa": 11}), ("seld_k_losses_strided", {"doa_loss": 4}),
       ("seld_k_losses_strided", {"doa_loss": -1}), ("seld_k_losses_strided", {"scratch": "misaligned"}),
       ("seld_k_losses_finalize", {"doa_loss": 4}), ("seld_k_losses_finalize", {"scratch": "misaligned"}),
       ("seld_k_agc", {"rank": 0}), ("seld_k_agc", {"rank": 5}), ("seld_k_agc", {"off": -1}), ("seld_k_agc", {"shape": (3, 0)}),
       ("seld_k_agc", {"shape": (1 << 20, 1 << 20)}),
       ("seld_k_act_bwd", {"n": 6}), ("seld_k_act_bwd", {"act": 0}), ("seld_k_act_bwd", {"act": 4}), ("seld_k_act_bwd", {"dy": "misaligned"}),
       ("seld_k_v1_couple_bwd", {"ld_sed": 3}), ("seld_k_v1_couple_bwd", {"ld_doa": 11}), ("seld_k_v1_couple_bwd", {"ld_sed": 0}),
       ("seld_k_time_expand", {"C": 6}), ("seld_k_time_expand", {"xe": "misaligned"}),
       ("seld_k_time_fold", {"C": 6}), ("seld_k_time_fold", {"dxe": "misaligned"}),
       ("seld_k_mask_rows", {"F": 6}), ("seld_k_mask_rows", {"mask": "misaligned"}),
       ("seld_k_dropout4", {"n": 6}), ("seld_k_dropout4", {"rate": 1.0}), ("seld_k_dropout4", {"rate": -0.01}),
       ("seld_k_dropout4", {"rate": float("nan")}), ("seld_k_dropout4", {"in": "misaligned"})]


@pytest.fixture(scope="module")
def env(seld_lib):
    """(library, base address of the buffer every pointer argument gets, the buffer if a device is present)"""
    gpu = torch.cuda.is_available()
    buf = torch.full((BUF_FLOATS,), FILL, device="cuda") if gpu else None
    base = buf.data_ptr() if gpu else 1 << 20     # no device: never dereferenced, a launch fails first
    yield seld_lib, base, buf
    del buf


def _call(env, op, doa_loss=0, **over):
    from seld_amd import _lib
    lib, base, _ = env
    cfg = _lib.LossCfg(doa_loss, 1.0, 1000.0, 1.0, 0.0)
    args = []
    for name, kind, val in OPS[op]:
        v = over.get(name, val)
        if kind in "po":
            v = C.c_void_p(base + 4) if v == "misaligned" else C.c_void_p(base) if name not in over else v
        elif kind == "c":
            v = C.byref(cfg) if name not in over else v
        elif kind == "h":
            v = (C.c_int64 * 4)(*v) if v is not None else None
        args.append(v)
    return getattr(lib, op)(*args)


def _got_through(env, rc):
    """past every refusal: SELD_OK with a device, the failed launch's SELD_ERR_HIP without one"""
    return rc == 0 if env[2] is not None else rc == HIP


def _unwritten(env):
    if env[2] is not None:
        torch.cuda.synchronize()
        assert bool((env[2] == FILL).all()), "a refused call wrote through a caller buffer"


def _null_and_size_cases():
    for op, spec in OPS.items():
        for name, kind, _ in spec:
            if kind in "pch":
                yield op, {name: None}
            elif kind == "s":
                yield op, {name: 0}
                yield op, {name: -1}


_ID = lambda v: v if isinstance(v, str) else ",".join(f"{k}={v[k]}" for k in v)


@pytest.mark.parametrize("op,bad", list(_null_and_size_cases()) + BAD, ids=_ID)
def test_refusals_come_first_and_write_nothing(env, op, bad):
    assert _call(env, op, **bad) == INVALID
    _unwritten(env)


@pytest.mark.parametrize("op", sorted(OPS))
def test_base_call_is_valid(env, op):
    """The unmodified call reaches its launch, so every refusal above is the bad argument's; so does the call with every optional pointer NULL
    (the losses without gradients, the coupling without the caller's copy) and the losses in every mode, deferred or not.  Runs behind the
    refusals: with a device these calls write the shared buffer."""
    assert _got_through(env, _call(env, op))
    assert _got_through(env, _call(env, op, **{n: None for n, kind, _ in OPS[op] if kind == "o"}))
    if op.startswith("seld_k_losses"):
        for mode in range(4):
            assert _got_through(env, _call(env, op, doa_loss=mode))
    if op == "seld_k_losses_strided":
        assert _got_through(env, _call(env, op, defer_finalize=1, ld_sed=4, ld_doa=12))
    if op == "seld_k_agc":
        for rank, shape in ((1, (5,)), (3, (2, 3, 4)), (4, (2, 2, 3, 4))):
            assert _got_through(env, _call(env, op, rank=rank, shape=shape))
    if env[2] is not None:
        torch.cuda.synchronize()
        env[2].fill_(FILL)


# ------------------------------------------------------------------------------------------------ the reference's own identities
def test_bce_restatement_equals_the_oracles_off_the_upper_clip_and_differs_on_it():
    """bce_f32_bounds is seldnet_oracle.bce wherever nothing is clipped from above; on one element at p = 0.99999994 with y = 0 the float32
    bounds give -log(2^-23 + 1e-7), the float64 ones -log(2e-7): 6e-3 of the value apart"""
    rng = np.random.default_rng(0)
    p = T.t64(torch.sigmoid(T.t64(rng.standard_normal(5000) * 3)).numpy().astype(np.float32))
    y = T.t64(rng.random(5000) < 0.1)
    assert float(p.max()) < T.BCE_HI
    assert abs(float(T.bce_f32_bounds(y, p)) / float(O.bce(y, p)) - 1) < 1e-9
    p1, y0 = T.t64(np.float32([0.99999994])), T.t64([0.0])
    a, b = float(T.bce_f32_bounds(y0, p1)), float(O.bce(y0, p1))
    print(f"[oracle] BCE element at p = 0.99999994, y = 0: float32 bounds {a:.5f}, float64 bounds {b:.5f}, apart {abs(a - b) / a:.2e}")
    assert 5e-3 < abs(a - b) / a < 7e-3
    assert T.BCE_HI == 1 - 2.0 ** -23 and abs(T.BCE_LO - 1e-7) < 2e-15


@pytest.mark.parametrize("ks", T.TIME_KS)
@pytest.mark.parametrize("B,S,Cc", T.TIME_SHAPES)
def test_expand_and_fold_are_transposes_and_expand_is_conv1d_same(B, S, Cc, ks):
    x, y, _ = (a.astype(np.float64) for a in T.time_case(B, S, Cc, ks))
    xe, fy = T.time_expand_ref(x, ks), T.time_fold_ref(y, ks)
    assert abs((xe * y).sum() - (x * fy).sum()) <= 1e-12 * np.abs(xe * y).sum()
    K = np.random.default_rng(ks).standard_normal((ks, Cc, 5))
    ref = O.conv1d_same(T.t64(x), T.t64(K), 0).numpy()
    assert rel_err(xe @ K.reshape(ks * Cc, 5), ref) <= 1e-13
    if ks == 2 and S >= 2:       # an even kernel's extra pad is behind: tap 0 reads the row itself, tap 1 the next one
        assert np.array_equal(xe[:, :, :Cc], x) and np.array_equal(xe[:, :-1, Cc:], x[:, 1:]) and not xe[:, -1, Cc:].any()


@pytest.mark.parametrize("mode", sorted(T.LOSS_MODES))
@pytest.mark.parametrize("rows,nc", T.V1_SHAPES)
def test_coupling_gradient_closed_form_is_autograd(rows, nc, mode):
    sed, doa1, ys, yd = T.v1_inputs(rows, nc)
    a, b = T.v1_bwd_ref(sed, doa1, ys, yd, mode), T.v1_bwd_ref(sed, doa1, ys, yd, mode, closed_form=True)
    for k in a:
        assert rel_err(b[k], a[k]) <= 1e-12, k


# ------------------------------------------------------------------------------------------------ float32 room under every bar
def _ratio(name, got, ref, tol):
    r = rel_err(got, ref) / tol
    print(f"[f32 / bar] {name:44s} {r:.3f}  (rel_err {r * tol:.2e})")
    assert r <= 0.5, f"{name}: a float32 evaluation of the reference uses {r:.2f} of the bar"


@pytest.mark.parametrize("mode", sorted(T.LOSS_MODES))
@pytest.mark.parametrize("B,S,nc", T.LOSS_SHAPES)
def test_float32_losses_stay_within_half_of_the_bars(B, S, nc, mode):
    sed, doa, ys, yd = T.loss_inputs(B, S, nc)
    assert T.tie_mask(doa, yd).sum() >= 2 and ((doa == 0) & (yd == 0)).any()
    assert (ys == 1).any() and (ys == 0).any() and (doa <= 0).any() and (yd <= 0).any() and not (doa == np.float32(1e-7)).any()
    ref, f32 = T.losses_ref(sed, doa, ys, yd, mode), T.losses_ref(sed, doa, ys, yd, mode, dtype=torch.float32)
    for k, tol in T.TOL.items():
        _ratio(f"losses {mode} {B, S, nc} {k}", f32[k], ref[k], tol)
    if mode == "MAE":
        assert not ref["ddoa_pre"][T.tie_mask(doa, yd)].any()
    if B * S > 4096:      # the 65th workgroup holds one row: without its partial sloss misses ten bars, so a finalize that stops at 64 cannot pass
        flat = [a.reshape(1, B * S, -1)[:, :-1] for a in (sed, doa, ys, yd)]
        short = T.losses_ref(*flat, mode)["sloss"][0] * (B * S - 1) / (B * S)
        assert 1 - short / ref["sloss"][0] >= 10 * T.TOL["sloss"]


def test_float32_bce_boundary_stays_within_half_of_the_bars():
    sed, ys, blocked = T.bce_boundary_case()
    doa, yd = np.zeros((1, 2, 36), np.float32), np.zeros((1, 2, 36), np.float32)
    ref, f32 = T.losses_ref(sed, doa, ys, yd, "MSE"), T.losses_ref(sed, doa, ys, yd, "MSE", dtype=torch.float32)
    assert blocked.sum() == 12 and not ref["dsed_pre"][blocked].any() and ref["dsed_pre"][~blocked].all()
    _ratio("BCE boundary sloss", f32["sloss"], ref["sloss"], T.TOL["sloss"])
    _ratio("BCE boundary dsed_pre", f32["dsed_pre"], ref["dsed_pre"], T.TOL["dsed_pre"])


@pytest.mark.parametrize("step", T.ADAM_STEPS)
@pytest.mark.parametrize("n", T.ADAM_NS)
def test_float32_adam_stays_within_half_of_the_bar(n, step):
    th, g, m, v, z = T.adam_case(n, step)
    for name, a, b in zip(("theta", "m", "v"), T.adam_ref(th, g, m, v, step, dtype=torch.float32), T.adam_ref(th, g, m, v, step)):
        _ratio(f"adam {name} n={n} step={step}", a, b, 1e-6)
    assert np.array_equal(T.adam_ref(th, g, m, v, step)[0][z], th[z].astype(np.float64))


@pytest.mark.parametrize("shape", T.AGC_SHAPES, ids=str)
def test_agc_cases_keep_their_margin_take_both_branches_and_leave_float32_room(shape):
    """the decision gn < max_norm is discontinuous: every unit of every case lies outside [0.9, 1.1] of it in float64, so float32 sums cannot
    flip one and no unit needs excluding; half of the units of every variable are clipped; the forced units are what they claim"""
    th, g, clip = T.agc_case(shape)
    rows, cols = T.agc_rows_cols(shape)
    ratio = T.agc_ratio(th, g)
    assert ((ratio < 0.9) | (ratio > 1.1)).all()
    assert np.array_equal(ratio > 1, clip)
    ref = T.agc_ref(th, g)
    changed = (ref != g.astype(np.float64)).reshape(rows, cols).any(axis=0)
    assert np.array_equal(changed, clip)
    if cols >= 8:
        assert 1 / 3 <= clip.mean() <= 2 / 3
        g2, t2 = g.reshape(rows, cols), th.reshape(rows, cols)
        assert not g2[:, 1].any() and not t2[:, 2:4].any() and clip[2] != clip[3]
        k = 2 if clip[2] else 3
        assert abs(np.sqrt((ref.reshape(rows, cols)[:, k] ** 2).sum()) / 1e-5 - 1) < 1e-6      # clipped to the ceiling of all-zero parameters
    e = T.unit_err(T.agc_f32(th, g), ref)
    tol = T.agc_tol(shape)
    print(f"[f32 / bar] agc {str(shape):20s} unit {rows:5d} elements: float32 serial error {e:.3e}, bar {tol:.3e}, ratio {e / tol:.3f}")
    assert e <= 0.5 * tol and tol <= T.AGC_TOL_MAX


def test_agc_rank_one_cases_take_one_branch_each():
    assert sorted(bool(T.agc_case(s)[2][0]) for s in T.AGC_SHAPES if len(s) == 1) == [False, True]


@pytest.mark.parametrize("act", [1, 2, 3])
@pytest.mark.parametrize("n", T.ACT_NS)
def test_float32_act_bwd_stays_within_half_of_the_bar(n, act):
    y, dy = T.act_case(n, act)
    ref = T.act_bwd_ref(y, dy, act)
    _ratio(f"act_bwd act={act} n={n}", T.act_bwd_ref(y, dy, act, np.float32), ref, 1e-6)
    ends = (y == 0) | (y == 1) if act != 2 else np.abs(y) == 1
    assert ends.sum() >= 2 and not ref[ends].any()


@pytest.mark.parametrize("rows,nc", T.V1_SHAPES)
def test_float32_coupling_stays_within_half_of_the_bars(rows, nc):
    sed, doa1, ys, yd = T.v1_inputs(rows, nc)
    _ratio(f"v1 fwd {rows, nc}", T.v1_fwd_ref(sed, doa1, torch.float32), T.v1_fwd_ref(sed, doa1), 2e-6)
    for mode in sorted(T.LOSS_MODES):
        a, b = T.v1_bwd_ref(sed, doa1, ys, yd, mode, dtype=torch.float32, closed_form=True), T.v1_bwd_ref(sed, doa1, ys, yd, mode)
        for k in b:
            _ratio(f"v1 bwd {mode} {rows, nc} {k}", a[k], b[k], 1e-4)


@pytest.mark.parametrize("rows,S,F", T.MASK_SHAPES)
def test_float32_mask_rows_stays_within_half_of_the_bar(rows, S, F):
    x, mask, prev = T.mask_rows_case(rows, S, F)
    assert (mask == 0).any() or rows == 1
    _ratio(f"mask_rows accumulate {rows, S, F}", T.mask_rows_ref(x, mask, S, prev, np.float32), T.mask_rows_ref(x, mask, S, prev), 1e-6)
    # without accumulate: one product, exact in float64, so the float32 result is its rounding and the GPU test asks for the bits
    assert np.array_equal(T.mask_rows_ref(x, mask, S, None, np.float32), T.mask_rows_ref(x, mask, S).astype(np.float32))


def test_dropout_reference_scale_and_mask():
    """float32(1 / (1 - rate)) is the kernel's 1.f / (1.f - rate) at the three rates; the mask is dropout_mask's; the kept share is 1 - rate"""
    for rate in T.DROP_RATES:
        assert np.float32(1) / (np.float32(1) - np.float32(rate)) == np.float32(1.0 / (1.0 - float(np.float32(rate))))
        v = np.ones(1028, np.float32)
        keep, out = T.dropout4_ref(v, rate, T.DROP_SEED, *T.DROP_STREAMS[0])
        assert np.array_equal(out.astype(np.float64), O.dropout_mask((1028,), rate, T.DROP_SEED, *T.DROP_STREAMS[0], torch.float64).numpy().astype(np.float32))
        assert abs(keep.mean() - (1 - rate)) < 0.05
    assert not np.array_equal(T.dropout4_ref(v, 0.5, T.DROP_SEED, *T.DROP_STREAMS[0])[0], T.dropout4_ref(v, 0.5, T.DROP_SEED, *T.DROP_STREAMS[1])[0])


# ------------------------------------------------------------------------------------------------ every kernel has a test
def test_every_kernel_of_loss_adam_is_named_by_a_gpu_test():
    src = open(os.path.join(ROOT, "seld_amd", "csrc", "loss_adam.hip")).read()
    kernels = re.findall(r"__global__\s+(?:__launch_bounds__\(\d+\)\s+)?void\s+(\w+)\s*\(", src)
    assert len(kernels) >= 15 and len(kernels) == len(set(kernels)) == src.count("__global__")      # the pattern misses no kernel
    assert sorted(kernels) == sorted(T.COVERAGE), "a kernel of loss_adam.hip has no entry in step_tail_oracle.COVERAGE, or an entry has no kernel"
    for k, tests in T.COVERAGE.items():
        assert tests
        for t in tests:
            fn, name = t.split("::")
            body = open(os.path.join(ROOT, "tests", fn)).read()
            assert fn.endswith("_gpu.py") and re.search(r"^def %s\(" % re.escape(name), body, flags=re.M), f"{k}: {t} does not exist"
