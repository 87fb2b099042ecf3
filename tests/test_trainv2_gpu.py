"""The trainv2 recipe on the GPU against the fp64 oracle (tests/trainv2_oracle.py): the loss kernel, the regulariser + AGC + AdaBelief
stage, one full v2 step through a context, SWA, and the untouched train.py path.  Error metric: tests/helpers.py::check
(max |a - b| / max |b| per tensor) at the project's 1e-4."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import trainv2_oracle as V
from helpers import check, dev, ptr

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ 1. seld_k_losses_v2
def _loss_case(B, S, nc, seed):
    rng = np.random.default_rng(seed)
    sed = rng.uniform(0.02, 0.98, (B, S, nc)).astype(np.float32)
    special = np.array([0.0, 1e-8, 1.0 - 1e-8, 1.0], np.float32)           # outside the clip: the gradient is exactly 0 there
    idx = rng.choice(B * S * nc, 8, replace=False)
    sed.reshape(-1)[idx] = np.tile(special, 2)
    y_sed = (rng.random((B, S, nc)) < 0.3).astype(np.float32)
    y_sed.reshape(-1)[idx[:4]] = [0, 1, 0, 1]                              # both label values meet both ends
    y_sed.reshape(-1)[idx[4:]] = [1, 0, 1, 0]
    vec = rng.standard_normal((B, S, 3, nc))
    vec /= np.linalg.norm(vec, axis=2, keepdims=True)
    y_doa = (vec * y_sed[:, :, None, :]).reshape(B, S, 3 * nc).astype(np.float32)
    zero_rows = [(0, 1), (B - 1, S - 1)]                                   # rows without any label: m = 0
    for b, s in zero_rows:
        y_doa[b, s] = 0.0
    doa = np.tanh(rng.standard_normal((B, S, 3 * nc))).astype(np.float32)
    w = rng.uniform(0.3, 3.0, nc).astype(np.float32)
    return sed, doa, y_sed, y_doa, w, idx, zero_rows


@pytest.mark.parametrize("ls", [0.0, 0.1])
@pytest.mark.parametrize("sed_loss", ["BCE", "focal"])
@pytest.mark.parametrize("B,S,nc", [(2, 10, 12), (4, 16, 14), (5, 13, 5)])      # 20 rows, 64 (one full workgroup), 65; nc % 4 = 0, 2, 1
def test_losses_v2(seld_lib, B, S, nc, sed_loss, ls):
    from seld_amd import _lib
    sed, doa, y_sed, y_doa, w, idx, zero_rows = _loss_case(B, S, nc, seed=100 + nc)
    lw = (1.0, 1000.0)
    ref = V.losses_v2_pre_grads(sed, doa, y_sed, y_doa, w, sed_loss=sed_loss, loss_weights=lw, ls=ls)
    cfg = _lib.V2Cfg(_lib.SELD_SED_BCE if sed_loss == "BCE" else _lib.SELD_SED_FOCAL, lw[0], lw[1], ls, 0.25, 2.0)
    for i in range(nc):
        cfg.cls_weights[i] = float(w[i])
    d = [dev(a) for a in (sed, doa, y_sed, y_doa)]
    outs = []
    for _ in range(2):
        sl, dl = torch.full((1,), float("nan"), device="cuda"), torch.full((1,), float("nan"), device="cuda")
        gs, gd = torch.full((B, S, nc), float("nan"), device="cuda"), torch.full((B, S, 3 * nc), float("nan"), device="cuda")
        assert seld_lib.seld_k_losses_v2(*[ptr(t) for t in d], C.byref(cfg), ptr(sl), ptr(dl), ptr(gs), ptr(gd), B, S, nc) == 0
        outs.append([t.cpu().numpy() for t in (sl, dl, gs, gd)])
    sl, dl, gs, gd = outs[0]
    check(f"losses_v2 sloss {sed_loss} ls={ls}", sl, ref["sloss"].reshape(1))
    check(f"losses_v2 dloss {sed_loss} ls={ls}", dl, ref["dloss"].reshape(1))
    check(f"losses_v2 dsed_pre {sed_loss} ls={ls}", gs, ref["dsed_pre"])
    check(f"losses_v2 ddoa_pre {sed_loss} ls={ls}", gd, ref["ddoa_pre"])
    assert (gs.reshape(-1)[idx] == 0).all() and (ref["dsed_pre"].reshape(-1)[idx] == 0).all()
    for b, s in zero_rows:
        assert (gd[b, s] == 0).all()
    for a, b in zip(outs[0], outs[1]):
        assert a.tobytes() == b.tobytes()
    # without gradient outputs the values are the same
    sl2, dl2 = torch.full((1,), float("nan"), device="cuda"), torch.full((1,), float("nan"), device="cuda")
    assert seld_lib.seld_k_losses_v2(*[ptr(t) for t in d], C.byref(cfg), ptr(sl2), ptr(dl2), None, None, B, S, nc) == 0
    assert sl2.cpu().numpy().tobytes() == sl.tobytes() and dl2.cpu().numpy().tobytes() == dl.tobytes()


# ------------------------------------------------------------------------------------------------ 2. seld_k_reg_agc_adabelief
SHAPES = [(3, 3, 8, 12), (12,), (1, 20, 12), (130,), (5, 7), (1500, 3)]      # ranks 4, 1, 3, 1, 2, 2; offsets 0, 864, 876, 1116, 1246 (% 4 = 2), 1281 (% 4 = 1)
REG = [1, 0, 1, 0, 1, 0]


def _rows_cols(shape):
    if len(shape) == 1:
        return shape[0], 1
    if len(shape) == 2:
        return shape
    if len(shape) == 3:
        return shape[0], shape[1] * shape[2]
    return shape[0] * shape[1] * shape[2], shape[3]


def _opt_weights(seed):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.standard_normal(int(np.prod(s))) * 0.2 for s in SHAPES]).astype(np.float32)


def _opt_grads(th, seed, step):
    """Per unit of the CURRENT weights `th`, a gradient whose norm is 0.3 x or 3 x the unit's max_norm = max(|w_unit|, 1e-3) * 0.01 (chosen at
    random): the fp64 oracle clips the second kind and not the first.  The regulariser's 2 l2 w moves a ratio by at most 0.2."""
    rng = np.random.default_rng(seed + 17 * step)
    g, off = [], 0
    for shape in SHAPES:
        rows, cols = _rows_cols(shape)
        w = np.asarray(th[off:off + rows * cols], np.float64).reshape(rows, cols)
        d = rng.standard_normal((rows, cols))
        target = np.where(rng.random(cols) < 0.5, 0.3, 3.0) * np.maximum(np.linalg.norm(w, axis=0), 1e-3) * 0.01
        g.append((d * (target / np.linalg.norm(d, axis=0))).reshape(-1))
        off += rows * cols
    return np.concatenate(g).astype(np.float32)


def test_opt_case_decisions_are_safe_on_the_cpu():
    """(collected with this file, but needs no device) three oracle steps per l2: every step has clipped and unclipped units and none within
    1e-3 of the decision — the seed was chosen so."""
    for l2 in (0.0, 1e-3):
        th = _opt_weights(5).astype(np.float64)
        m, v = np.zeros_like(th), np.zeros_like(th)
        for step in (1, 2, 3):
            r = V.reg_agc_adabelief(th, _opt_grads(th, 5, step), m, v, SHAPES, REG, step, l2=l2)
            assert (r["ratio"] < 1).any() and (r["ratio"] >= 1).any() and np.abs(r["ratio"] - 1).min() > 1e-3
            th, m, v = r["theta"].astype(np.float32), r["m"].astype(np.float32), r["v"].astype(np.float32)


@pytest.mark.parametrize("clip_factor", [0.01, 0.0])
@pytest.mark.parametrize("l2", [0.0, 1e-3])
def test_reg_agc_adabelief(seld_lib, l2, clip_factor):
    """Three steps with the moments carried on the device; steps 1 and 3 are compared.  The oracle starts each step from the device's own
    float32 state, so a step's figures are that step's arithmetic alone.  m, v, the written-back gradient and the update at 1e-4;
    tests/test_kernels_gpu.py::test_adam has no floor-aware bar for small second moments (it compares v at a plain relative bar), so
    none is added here: v is checked like the rest.  The update is compared as theta_after - theta_before: with |theta| < 1 and updates
    of ~lr / 0.9 the float32 storage of theta contributes at most 2^-25 / 1.1e-3 = 2.7e-5 of the bar."""
    n = sum(int(np.prod(s)) for s in SHAPES)
    rc = [_rows_cols(s) for s in SHAPES]
    off = np.cumsum([0] + [r * c for r, c in rc])[:-1]
    assert list(off) == [0, 864, 876, 1116, 1246, 1281] and n == 5781
    nv = len(SHAPES)
    args = ((C.c_int64 * nv)(*[int(o) for o in off]), (C.c_int32 * nv)(*[r for r, _ in rc]), (C.c_int32 * nv)(*[c for _, c in rc]), (C.c_int32 * nv)(*REG))
    th0 = _opt_weights(5)
    assert np.abs(th0).max() < 1.0
    td, md, vd = dev(th0), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    for step in (1, 2, 3):
        th_b, m_b, v_b = td.cpu().numpy(), md.cpu().numpy(), vd.cpu().numpy()
        g = _opt_grads(th_b, 5, step)
        ref = V.reg_agc_adabelief(th_b, g, m_b, v_b, SHAPES, REG, step, lr=1e-3, l2=l2, clip_factor=clip_factor)
        if clip_factor > 0:
            r = ref["ratio"]
            assert (r < 1).any() and (r >= 1).any() and np.abs(r - 1).min() > 1e-3      # no fp32 evaluation can flip a decision
        gd = dev(g)
        assert seld_lib.seld_k_reg_agc_adabelief(ptr(td), ptr(gd), ptr(md), ptr(vd), n, nv, *args, 1e-3, 0.9, 0.999, 1e-7, l2, clip_factor, step) == 0
        if step == 2:
            continue
        tag = f"step {step} l2={l2} clip={clip_factor}"
        check(f"adabelief g' {tag}", gd.cpu().numpy(), ref["g"])
        check(f"adabelief m {tag}", md.cpu().numpy(), ref["m"])
        check(f"adabelief v {tag}", vd.cpu().numpy(), ref["v"])
        check(f"adabelief update {tag}", td.cpu().numpy().astype(np.float64) - th_b, ref["theta"] - th_b)
        if clip_factor == 0 and l2 == 0:
            assert gd.cpu().numpy().tobytes() == g.tobytes()
        for k, (shape, o) in enumerate(zip(SHAPES, off)):      # and per variable, so that a small one cannot hide behind a large one
            sl = slice(int(o), int(o) + int(np.prod(shape)))
            check(f"adabelief g' var {k} {tag}", gd.cpu().numpy()[sl], ref["g"][sl])
            check(f"adabelief update var {k} {tag}", td.cpu().numpy().astype(np.float64)[sl] - th_b[sl], (ref["theta"] - th_b)[sl])


# ------------------------------------------------------------------------------------------------ 3. one full v2 step through a context
def _per_var(model, name, got, ref, tol=1e-4):
    """tests/test_model_gpu.py::_per_var: every variable at the bar, except the conv biases in front of training-mode BatchNorm, whose
    gradient is exactly 0 in exact arithmetic (rounding noise on both sides: held against the scale of the whole gradient)."""
    for n, off, sh in model.variables:
        k = int(np.prod(sh))
        if n.startswith("conv") and n.endswith("bias"):
            assert np.abs(got[off:off + k]).max() <= 1e-3 * max(1.0, np.abs(ref).max()), n
            continue
        check(f"{name} {n}", got[off:off + k], ref[off:off + k], tol)


def _check_update(name, w0, w1, ref_w1, tol=1e-4):
    """theta_after - theta_before against the oracle's update.  The update is only observable through the float32 weight it was added to:
    that storage rounds by up to half an ulp, 2^-24 max|w|, whatever the kernel does, so the bar is tol * max|update| plus that half ulp
    (the form of tests/test_model_gpu.py::_check_adam_first_step).  For a variable whose updates are ~lr the second term is the smaller."""
    got, ref = w1.astype(np.float64) - w0, ref_w1 - w0
    err, bar = np.abs(got - ref).max(), tol * np.abs(ref).max() + 2.0 ** -24 * np.abs(w0).max()
    print(f"[parity] {name:40s} max |update - ref| = {err:.3e}  bar {bar:.3e}  (|update|max={np.abs(ref).max():.3e})")
    assert np.isfinite(w1).all() and err <= bar, (name, err, bar)


def _v2_direct(model, x, ys, yd, cfg, l2, lr=1e-3):
    """seld_set_regularized + seld_train_fwd_bwd_v2 + seld_v2_opt_step, called directly -> everything the step produced."""
    from seld_amd import _lib, train, trainv2
    flags = (C.c_int32 * len(model.variables))(*[int(trainv2.is_regularized(n)) for n, _, _ in model.variables])
    _lib.check(model.lib.seld_set_regularized(model.ctx, flags, len(model.variables)), model.ctx)
    xd = model._prep(x)
    ysd, ydd = train._labels(model, (ys, yd), x.shape[0])
    sed, doa = model._outputs(x.shape[0])
    sl, dl = torch.empty((), device="cuda"), torch.empty((), device="cuda")
    _lib.check(model.lib.seld_train_fwd_bwd_v2(model.ctx, xd.data_ptr(), ysd.data_ptr(), ydd.data_ptr(), C.byref(cfg), sed.data_ptr(), doa.data_ptr(),
                                               sl.data_ptr(), dl.data_ptr()), model.ctx)
    g_raw = model.get_grads()
    _lib.check(model.lib.seld_v2_opt_step(model.ctx, lr, 0.9, 0.999, 1e-7, l2, 0.01), model.ctx)
    w1, st1 = model.get_weights()
    m = np.empty(model.n_params, np.float32); v = np.empty(model.n_params, np.float32)
    _lib.check(model.lib.seld_get_adam_host(model.ctx, m.ctypes.data, v.ctypes.data, model.n_params), model.ctx)
    return {"sed": sed.cpu().numpy(), "doa": doa.cpu().numpy(), "sloss": sl.cpu().numpy(), "dloss": dl.cpu().numpy(), "g_raw": g_raw,
            "g": model.get_grads(), "w": w1, "state": st1, "m": m, "v": v}


@pytest.mark.parametrize("which,sed_loss", [("seldnet", "BCE"), ("seldnet_v1", "focal")])
def test_full_v2_step(seldnet_config, which, sed_loss):
    """Outputs, both losses and every variable's gradient against the fp64 oracle.  The clip is discontinuous in the gradient (as
    tests/test_model_gpu.py::test_train_step_agc notes), so the optimizer stage — regulariser, clip, AdaBelief: the written-back gradient
    and every variable's update — is compared with the oracle's stage applied to the library's own raw gradient (the clip itself is
    continuous where a decision flips: the factor is 1 there).  The update over the whole buffer is held to the plain 1e-4 (|w| < 2:
    float32 storage of the new weight contributes at most 2^-24 / 1.1e-3 = 5.4e-5 of it), per variable to _check_update's bar.  Then the
    same step through seld_amd.trainv2 gives the same bits as the direct calls."""
    from oracle import seldnet_oracle as O
    from seld_amd import _lib, losses, models, trainv2
    B, T, l2, ls = 2, 50, 1e-3, 0.1
    spec = O.Spec.from_config(seldnet_config)
    spec.output_coupling = which == "seldnet_v1"
    w, st = O.random_weights(spec, 0)
    x, ys, yd = O.synthetic_batch(B, T)
    wc = trainv2.default_cls_weights()
    build = lambda: getattr(models, which)((B, T, 64, 7), copy.deepcopy(seldnet_config))
    model = build()
    assert model.n_classes == 12
    model.set_weights(w, st)
    sel = losses.BinaryCrossentropy() if sed_loss == "BCE" else losses.focal_loss
    cfg = trainv2._v2_cfg(sel, (1.0, 1000.0), ls, wc)
    got = _v2_direct(model, x, ys, yd, cfg, l2)
    ref = V.train_step_v2(spec, w, st, x, ys, yd, wc, sed_loss=sed_loss, loss_weights=(1.0, 1000.0), ls=ls)
    for k in ("sed", "doa", "sloss", "dloss"):
        check(f"v2 step {which} {k}", got[k], ref[k])
    check(f"v2 step {which} BN moving stats", got["state"], ref["new_state"])
    _per_var(model, f"v2 step {which} grad", got["g_raw"], ref["grad"])
    shapes = [sh for _, _, sh in model.variables]
    reg = [int(V.is_regularized(n)) for n, _, _ in model.variables]
    assert sum(reg) == 7
    opt = V.reg_agc_adabelief(w, got["g_raw"], np.zeros_like(w), np.zeros_like(w), shapes, reg, 1, lr=1e-3, l2=l2, clip_factor=0.01)
    print(f"[parity] v2 step {which}: {int((opt['ratio'] >= 1).sum())} of {opt['ratio'].size} units clipped")
    assert (opt["ratio"] >= 1).any() and (opt["ratio"] < 1).any()
    assert np.abs(w).max() < 2.0
    check(f"v2 step {which} update, all variables", got["w"].astype(np.float64) - w, opt["theta"] - w)
    for n, off, sh in model.variables:
        sl_ = slice(off, off + int(np.prod(sh)))
        check(f"v2 step {which} consumed grad {n}", got["g"][sl_], opt["g"][sl_])
        check(f"v2 step {which} m {n}", got["m"][sl_], opt["m"][sl_])
        _check_update(f"v2 step {which} update {n}", w[sl_], got["w"][sl_], opt["theta"][sl_])
    del model
    # the Python surface: generate_trainstep + AdaBelief on a fresh context
    model = build()
    model.set_weights(w, st)
    assert trainv2.apply_kernel_regularizer(model, l2) is model
    step = trainv2.generate_trainstep(sel, losses.MMSE_with_cls_weights, (1, 1000), label_smoothing=ls)
    y_p, sl, dl = step(model, x, (ys, yd), trainv2.AdaBelief(1e-3))
    w1, st1 = model.get_weights()
    for name, a, b in (("sed", y_p[0].cpu().numpy(), got["sed"]), ("doa", y_p[1].cpu().numpy(), got["doa"]), ("sloss", sl.cpu().numpy(), got["sloss"]),
                       ("dloss", dl.cpu().numpy(), got["dloss"]), ("grad", model.get_grads(), got["g"]), ("weights", w1, got["w"]), ("state", st1, got["state"])):
        assert a.tobytes() == b.tobytes(), name
    ts = trainv2.generate_teststep(losses.BinaryCrossentropy(), losses.MMSE_with_cls_weights)
    ref_t = O.test_step(spec, w1, st1, x, ys, yd, "MMSE", dtype=torch.float64)
    y_t, sl_t, dl_t = ts(model, x, (ys, yd))
    check(f"v2 teststep {which} sloss", sl_t.cpu().numpy(), ref_t["sloss"])
    check(f"v2 teststep {which} dloss", dl_t.cpu().numpy(), ref_t["dloss"])


# ------------------------------------------------------------------------------------------------ 4. SWA
def test_swa(seldnet_config):
    from oracle import seldnet_oracle as O
    from seld_amd import _lib, models, trainv2
    spec = O.Spec.from_config(seldnet_config)
    model = models.seldnet((2, 50, 64, 7), seldnet_config)
    assert model.lib.seld_swa_apply(model.ctx) == -1 and model.lib.seld_swa_count(model.ctx) == 0      # SELD_ERR_INVALID before the first update
    swa = trainv2.SWA(model, start_epoch=3, swa_freq=2)
    ref_w = ref_s = None
    fired = []
    for epoch in range(8):
        w, st = O.random_weights(spec, 10 + epoch)
        model.set_weights(w, st)
        before = swa.cnt
        swa.on_epoch_end(epoch)
        if swa.cnt != before:
            fired.append(epoch)
            ref_w, ref_s = (w, st) if before == 0 else (V.swa_update(ref_w, w, before), V.swa_update(ref_s, st, before))
    assert fired == [e for e in range(8) if V.swa_fires(e, 3, 2)] == [2, 4, 6] and swa.cnt == 3
    swa.on_train_end()
    w1, st1 = model.get_weights()
    assert w1.tobytes() == ref_w.tobytes() and st1.tobytes() == ref_s.tobytes()


# ------------------------------------------------------------------------------------------------ 5. the existing paths are untouched
def test_v1_path_untouched_by_a_v2_step_elsewhere(seldnet_config):
    from oracle import seldnet_oracle as O
    from seld_amd import losses, models, train, trainv2
    B, T = 2, 50
    spec = O.Spec.from_config(seldnet_config)
    w, st = O.random_weights(spec, 0)
    x, ys, yd = O.synthetic_batch(B, T)

    def v1_step():
        model = models.seldnet((B, T, 64, 7), seldnet_config)
        model.set_weights(w, st)
        y_p, sl, dl = train.trainstep(model, x, (ys, yd), losses.BinaryCrossentropy(), losses.MMSE, (1.0, 1000.0), train.Adam(1e-3), True)
        out = [y_p[0].cpu().numpy(), y_p[1].cpu().numpy(), sl.cpu().numpy(), dl.cpu().numpy(), model.get_grads(), *model.get_weights()]
        del model
        return out

    first = v1_step()
    other = models.seldnet((B, T, 64, 7), seldnet_config)
    other.set_weights(w, st)
    trainv2.apply_kernel_regularizer(other, 1e-3)
    step = trainv2.generate_trainstep(losses.focal_loss, losses.MMSE_with_cls_weights, (1, 1000), 0.1)
    step(other, x, (ys, yd), trainv2.AdaBelief())
    trainv2.SWA(other, 1).on_epoch_end(0)
    second = v1_step()          # `other` is still alive
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes()
    # and on the SAME context the v1 step after a v2 step still runs its own loss stage (the deferred finalize is its own)
    other.set_weights(w, st)
    _, sl, dl = train.trainstep(other, x, (ys, yd), losses.BinaryCrossentropy(), losses.MMSE, (1.0, 1000.0), train.Adam(1e-3), True)
    assert sl.cpu().numpy().tobytes() == first[2].tobytes() and dl.cpu().numpy().tobytes() == first[3].tobytes()
