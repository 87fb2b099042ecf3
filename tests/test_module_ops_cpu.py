"""The seld_m_* module operators refuse bad arguments before they enqueue anything (include/seld_hip.h, module_ops.hip), checked
without a GPU: each call below is one valid call with ONE argument made bad (a required pointer NULL, a size 0 or -1, ...).  The
library loads without a device; a call that got as far as a launch there returns SELD_ERR_HIP instead of SELD_ERR_INVALID, so the
return code shows whether the refusal came first.  On a machine with a GPU the pointers are real device memory and the base call's
sizes stay inside it, so a call that wrongly launched would return SELD_OK and fail the same way.  Also: seld_m_conv_out, the
scratch-size functions and the bench's mother_stage arguments restated in tests/test_module_ops_gpu.py."""
import ctypes as C

import pytest
import torch

from seld_amd import _lib

INVALID, UNSUPPORTED, HIP = -1, -2, -3

# one valid call per operator: (argument name, kind, value).  kinds: p required pointer, o pointer that may be NULL, s size (refused at 0
# and -1), v anything else.  Pointer values are filled in by _args(); the sizes keep every buffer within BUF_FLOATS.
OPS = {
    "seld_m_im2col": [("x", "p", 0), ("col", "p", 0), ("B", "s", 1), ("H", "s", 2), ("W", "s", 2), ("C", "s", 2), ("kh", "s", 1),
                      ("kw", "s", 1), ("sh", "s", 1), ("sw", "s", 1)],
    "seld_m_col2im": [("dcol", "p", 0), ("dx", "p", 0), ("B", "s", 1), ("H", "s", 2), ("W", "s", 2), ("C", "s", 2), ("kh", "s", 1),
                      ("kw", "s", 1), ("sh", "s", 1), ("sw", "s", 1), ("accumulate", "v", 0)],
    "seld_m_gemm": [("A", "p", 0), ("Bm", "p", 0), ("bias", "o", 0), ("Cm", "p", 0), ("M", "s", 4), ("N", "s", 4), ("K", "s", 4),
                    ("transb", "v", 0), ("accumulate", "v", 0)],
    "seld_m_gemm_tn": [("A", "p", 0), ("Bm", "p", 0), ("Cm", "p", 0), ("colsum", "o", 0), ("slab", "p", 0), ("M", "s", 4), ("K1", "s", 4),
                       ("N", "s", 4), ("seq", "v", 0), ("shift", "v", 0)],
    "seld_m_bn_stats": [("z", "p", 0), ("npix", "s", 4), ("C", "s", 2), ("mean", "p", 0), ("var", "p", 0), ("scratch", "o", 0)],
    "seld_m_bn_apply": [("z", "p", 0), ("mean", "p", 0), ("var", "p", 0), ("gamma", "p", 0), ("beta", "p", 0), ("eps", "v", 1e-3),
                        ("out", "p", 0), ("npix", "s", 4), ("C", "s", 2), ("accumulate", "v", 0)],
    "seld_m_bn_moving": [("mean", "p", 0), ("var", "p", 0), ("mov_mean", "p", 0), ("mov_var", "p", 0), ("C", "s", 2), ("momentum", "v", 0.99),
                         ("count", "s", 8)],
    "seld_m_bn_bwd": [("z", "p", 0), ("dy", "p", 0), ("mean", "p", 0), ("var", "p", 0), ("gamma", "p", 0), ("eps", "v", 1e-3), ("dz", "p", 0),
                      ("dgamma", "p", 0), ("dbeta", "p", 0), ("npix", "s", 4), ("C", "s", 2), ("scratch", "o", 0)],
    "seld_m_act": [("x", "p", 0), ("y", "p", 0), ("n", "s", 8), ("kind", "v", 1)],
    "seld_m_act_bwd": [("x", "p", 0), ("dy", "p", 0), ("dx", "p", 0), ("n", "s", 8), ("kind", "v", 1), ("accumulate", "v", 0)],
    "seld_m_axpy": [("dst", "p", 0), ("src", "p", 0), ("n", "s", 8), ("alpha", "v", 0.5)],
    "seld_m_copy_channels": [("src", "p", 0), ("dst", "p", 0), ("rows", "s", 2), ("Cs", "s", 2), ("Cd", "s", 3), ("off", "v", 1), ("mode", "v", 0)],
    "seld_m_mean_hw": [("x", "p", 0), ("out", "p", 0), ("B", "s", 1), ("HW", "s", 2), ("C", "s", 2)],
    "seld_m_scale_hw": [("x", "p", 0), ("s", "p", 0), ("y", "p", 0), ("B", "s", 1), ("HW", "s", 2), ("C", "s", 2)],
    "seld_m_scale_hw_bwd_ds": [("x", "p", 0), ("dy", "p", 0), ("ds", "p", 0), ("B", "s", 1), ("HW", "s", 2), ("C", "s", 2)],
    "seld_m_scale_hw_bwd_dx": [("dy", "p", 0), ("s", "p", 0), ("dmean", "o", 0), ("dx", "p", 0), ("B", "s", 1), ("HW", "s", 2), ("C", "s", 2),
                               ("accumulate", "v", 0)],
    "seld_m_gru_fwd": [("gx_f", "p", 0), ("gx_b", "p", 0), ("U_f", "p", 0), ("U_b", "p", 0), ("brec_f", "p", 0), ("brec_b", "p", 0),
                       ("h_f", "p", 0), ("h_b", "p", 0), ("saved_f", "o", 0), ("saved_b", "o", 0), ("out", "o", 0), ("B", "s", 1), ("S", "s", 1),
                       ("units", "v", 128)],
    "seld_m_gru_bwd": [("dout", "p", 0), ("h_f", "p", 0), ("h_b", "p", 0), ("saved_f", "p", 0), ("saved_b", "p", 0), ("U_f", "p", 0),
                       ("U_b", "p", 0), ("dgx_f", "p", 0), ("dgx_b", "p", 0), ("dgh_f", "p", 0), ("dgh_b", "p", 0), ("B", "s", 1), ("S", "s", 1),
                       ("units", "v", 128)],
    "seld_m_losses": [("sed", "p", 0), ("doa", "p", 0), ("y_sed", "p", 0), ("y_doa", "p", 0), ("cfg", "p", 0), ("sloss", "p", 0),
                      ("dloss", "p", 0), ("dsed_pre", "o", 0), ("ddoa_pre", "o", 0), ("scratch", "p", 0), ("B", "s", 1), ("S", "s", 1),
                      ("nc", "s", 2)],
    "seld_m_adam": [("theta", "p", 0), ("g", "p", 0), ("m", "p", 0), ("v", "p", 0), ("n", "s", 8), ("lr", "v", 1e-3), ("beta1", "v", 0.9),
                    ("beta2", "v", 0.999), ("eps", "v", 1e-7), ("step", "s", 1)],
}
BUF_FLOATS = 1 << 18      # the largest base call: the GRU's U [128, 384] and the BatchNormalization scratch (1024 x 4 x 2)


@pytest.fixture(scope="module")
def env(seld_lib):
    """(library, pointer for every buffer, loss config, whether a device is present)"""
    gpu = torch.cuda.is_available()
    buf = torch.zeros(BUF_FLOATS, device="cuda") if gpu else None
    p = C.c_void_p(buf.data_ptr()) if gpu else C.c_void_p(1 << 20)     # no device: never dereferenced, a launch fails first
    cfg = _lib.LossCfg(0, 1.0, 1000.0, 1.0, 0.0)
    yield seld_lib, p, cfg, gpu
    del buf


def _args(env, op, **over):
    lib, p, cfg, _ = env
    out = []
    for name, kind, val in OPS[op]:
        v = over.get(name, val)
        if kind in "po" and name not in over:
            v = C.byref(cfg) if name == "cfg" else p
        out.append(v)
    return out + [None]      # the stream: the null stream


def _call(env, op, **over):
    return getattr(env[0], op)(*_args(env, op, **over))


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
    """The unmodified call gets as far as its launch — SELD_ERR_HIP without a device, SELD_OK on the placeholder buffer with one — so
    the refusals below are the bad argument's."""
    assert _call(env, op) == (0 if env[3] else HIP)
    if env[3]:
        torch.cuda.synchronize()


@pytest.mark.parametrize("op,bad", list(_cases()), ids=lambda v: v if isinstance(v, str) else ",".join(f"{k}={v[k]}" for k in v))
def test_refuses_null_pointer_and_size_below_one(env, op, bad):
    assert _call(env, op, **bad) == INVALID


def test_refuses_what_the_header_documents(env):
    # the concatenation piece must lie inside the destination row; only modes 0 and 1 exist
    assert _call(env, "seld_m_copy_channels", Cs=2, Cd=3, off=2) == INVALID
    assert _call(env, "seld_m_copy_channels", off=-1) == INVALID
    assert _call(env, "seld_m_copy_channels", mode=2) == INVALID
    assert _call(env, "seld_m_copy_channels", mode=-1) == INVALID
    # gemm_tn's sequences must tile the rows
    assert _call(env, "seld_m_gemm_tn", M=4, seq=3, shift=1) == INVALID
    assert _call(env, "seld_m_gemm_tn", seq=-1) == INVALID
    # unknown activation kinds
    for op in ("seld_m_act", "seld_m_act_bwd"):
        assert _call(env, op, kind=5) == INVALID
        assert _call(env, op, kind=-1) == INVALID
    # the recurrence exists for 128 units only: UNSUPPORTED, checked before anything else
    for op in ("seld_m_gru_fwd", "seld_m_gru_bwd"):
        for u in (64, 127, 129, 256, 0):
            assert _call(env, op, units=u) == UNSUPPORTED
        assert _call(env, op, units=256, B=0) == UNSUPPORTED


def test_conv_out_is_same_out():
    from oracle.modules_oracle import same_out
    lib = _lib.load()
    for n in list(range(1, 70)) + [599, 600, 601, 3000, 3001]:
        for s in range(1, 9):
            assert lib.seld_m_conv_out(n, s) == same_out(n, s), (n, s)
    for n, s in ((0, 1), (-1, 1), (5, 0), (5, -1)):
        assert lib.seld_m_conv_out(n, s) == INVALID


def test_scratch_sizes():
    """bn: 1 024 first-stage workgroups x [2][C] doubles; gemm_tn: 128 slabs of K1 x N + N floats; losses: 2 rows + 64, and the MMSE
    denominator after them (module_ops.hip, gemm.hip, loss_adam.hip)."""
    from test_module_ops_gpu import BNP_MAX_BLOCKS
    lib = _lib.load()
    for c in (1, 3, 96, 199, 257, 2048, 2049):
        assert lib.seld_m_bn_scratch(c) == BNP_MAX_BLOCKS * 2 * 2 * c
    for k1, n in ((1, 1), (63, 96), (927, 96), (4378, 384), (128, 384)):
        assert lib.seld_m_gemm_tn_scratch(k1, n) == 128 * (k1 * n + n)
    for r in (1, 14, 19200):
        assert lib.seld_m_losses_scratch(r) == 2 * r + 64 + 4
    for bad in (0, -1):
        assert lib.seld_m_bn_scratch(bad) == -1
        assert lib.seld_m_losses_scratch(bad) == -1
        assert lib.seld_m_gemm_tn_scratch(bad, 4) == -1
        assert lib.seld_m_gemm_tn_scratch(4, bad) == -1


def test_restated_bench_args_match_bench():
    import bench
    from test_module_ops_gpu import BENCH_B, BENCH_T, MOTHER_STAGE_ARGS, bench_shapes
    assert MOTHER_STAGE_ARGS == bench.MOTHER_STAGE_ARGS
    assert bench.mother_stage_leg.__defaults__[:2] == (BENCH_B, BENCH_T)
    sh = bench_shapes()
    assert sh["blocks"] == [((3000, 64, 7), (600, 22, 103)), ((600, 22, 103), (600, 22, 199))]
    assert sh["gru_in"] == 22 * 199
