"""The trainv2 recipe on composed models, on the device: the stream operators seld_v2_losses / seld_v2_opt / seld_v2_swa against the
seld_k_* entry points (bit for bit) and the fp64 oracle (tests/trainv2_oracle.py), seld_aug_v2 against a numpy restatement and the
add + transforms.mask path (bit for bit), and full v2 steps on models.conv_temporal and a composed models.seldnet against
tests/conv_temporal_oracle.py / oracle/modules_oracle.py under autograd.  Error metric: helpers.check at the project's 1e-4."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import conv_temporal_oracle as CT
import trainv2_composed_cases as K
import trainv2_oracle as V
from helpers import check, dev, ptr
from test_attention_gpu import _check_or_zero
from test_trainv2_gpu import _loss_case

pytestmark = pytest.mark.gpu

bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
same = lambda a, b: np.array_equal(bits(a), bits(b))


def _sp(stream):
    return C.c_void_p(stream.cuda_stream)


# ------------------------------------------------------------------------------------------------ 5. seld_v2_losses
@pytest.mark.parametrize("ls", [0.0, 0.1])
@pytest.mark.parametrize("sed_loss", ["BCE", "focal"])
@pytest.mark.parametrize("B,S,nc", [(2, 10, 12), (4, 16, 14), (5, 13, 13)])      # 20 rows, 64 (one full workgroup), 65; nc % 4 = 0, 2, 1
def test_m_losses_v2(seld_lib, B, S, nc, sed_loss, ls):
    from seld_amd import _lib
    sed, doa, y_sed, y_doa, w, _, _ = _loss_case(B, S, nc, seed=100 + nc)
    cfg = _lib.V2Cfg(_lib.SELD_SED_BCE if sed_loss == "BCE" else _lib.SELD_SED_FOCAL, 1.0, 1000.0, ls, 0.25, 2.0)
    for i in range(nc):
        cfg.cls_weights[i] = float(w[i])
    d = [dev(a) for a in (sed, doa, y_sed, y_doa)]
    new = lambda: [torch.full(s, float("nan"), device="cuda") for s in ((1,), (1,), (B, S, nc), (B, S, 3 * nc))]
    ref = new()
    assert seld_lib.seld_k_losses_v2(*[ptr(t) for t in d], C.byref(cfg), *[ptr(t) for t in ref], B, S, nc) == 0
    ref = [t.cpu().numpy() for t in ref]
    n_scr = int(seld_lib.seld_v2_losses_scratch(B * S))
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    for _ in range(2):
        out = new()
        scr = torch.full((n_scr + 64,), float("nan"), device="cuda")
        with torch.cuda.stream(stream):
            assert seld_lib.seld_v2_losses(*[ptr(t) for t in d], C.byref(cfg), *[ptr(t) for t in out], ptr(scr), B, S, nc, _sp(stream)) == 0
        stream.synchronize()
        assert bool(torch.isnan(scr[n_scr:]).all()), "wrote behind the scratch it asked for"
        for name, a, b in zip(("sloss", "dloss", "dsed_pre", "ddoa_pre"), out, ref):
            assert same(a.cpu().numpy(), b), name
    # without gradient outputs the losses are the same
    out = new()
    scr = torch.empty(n_scr, device="cuda")
    assert seld_lib.seld_v2_losses(*[ptr(t) for t in d], C.byref(cfg), ptr(out[0]), ptr(out[1]), None, None, ptr(scr), B, S, nc, None) == 0
    torch.cuda.synchronize()
    assert same(out[0].cpu().numpy(), ref[0]) and same(out[1].cpu().numpy(), ref[1])


# ------------------------------------------------------------------------------------------------ 6. seld_v2_opt
@pytest.mark.parametrize("clip_factor", [0.01, 0.0])
@pytest.mark.parametrize("l2", [0.0, 1e-3])
def test_m_v2_opt(seld_lib, l2, clip_factor):
    """Two consecutive steps on a plan built once, against seld_k_reg_agc_adabelief on copies of the same buffers (identical bits) and
    against the fp64 oracle started from the device's own float32 state (the bars of test_trainv2_gpu.test_reg_agc_adabelief: 1e-4 on m, v,
    the written-back gradient and the update)."""
    nv, n = len(K.OPT_SHAPES), K.OPT_N
    rc = [K.rows_cols(s) for s in K.OPT_SHAPES]
    args = ((C.c_int64 * nv)(*K.OPT_OFFSETS), (C.c_int32 * nv)(*[r for r, _ in rc]), (C.c_int32 * nv)(*[c for _, c in rc]), (C.c_int32 * nv)(*K.OPT_REG))
    plan = C.c_void_p()
    assert seld_lib.seld_v2_plan_create(n, nv, *args, C.byref(plan)) == 0 and plan.value
    stream = torch.cuda.Stream()
    try:
        th0 = K.opt_weights()
        assert np.abs(th0).max() < 1.0
        a = [dev(th0), None, torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")]      # theta, g, m, v of the stream operator
        b = [t.clone() if t is not None else None for t in a]                                    # and of seld_k_reg_agc_adabelief
        for step in (1, 2):
            th_b, m_b, v_b = (a[i].cpu().numpy() for i in (0, 2, 3))
            g = K.opt_grads(th_b, step)
            ref = V.reg_agc_adabelief(th_b, g, m_b, v_b, K.OPT_SHAPES, K.OPT_REG, step, lr=1e-3, l2=l2, clip_factor=clip_factor)
            if clip_factor > 0:
                assert K.ratios_are_safe(ref["ratio"])
            a[1], b[1] = dev(g), dev(g)
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                assert seld_lib.seld_v2_opt(plan, *[ptr(t) for t in a], 1e-3, 0.9, 0.999, 1e-7, l2, clip_factor, step, _sp(stream)) == 0
            stream.synchronize()
            assert seld_lib.seld_k_reg_agc_adabelief(*[ptr(t) for t in b], n, nv, *args, 1e-3, 0.9, 0.999, 1e-7, l2, clip_factor, step) == 0
            got = [t.cpu().numpy() for t in a]
            for name, x, y in zip(("theta", "g", "m", "v"), got, b):
                assert same(x, y.cpu().numpy()), f"step {step}: {name}"
            tag = f"step {step} l2={l2} clip={clip_factor}"
            check(f"m_v2_opt g' {tag}", got[1], ref["g"])
            check(f"m_v2_opt m {tag}", got[2], ref["m"])
            check(f"m_v2_opt v {tag}", got[3], ref["v"])
            check(f"m_v2_opt update {tag}", got[0].astype(np.float64) - th_b, ref["theta"] - th_b)
            if clip_factor == 0 and l2 == 0:
                assert same(got[1], g)
            for k, (shape, o) in enumerate(zip(K.OPT_SHAPES, K.OPT_OFFSETS)):      # per variable: a small one cannot hide behind a large one
                sl = slice(o, o + int(np.prod(shape)))
                check(f"m_v2_opt g' var {k} {tag}", got[1][sl], ref["g"][sl])
                check(f"m_v2_opt update var {k} {tag}", got[0].astype(np.float64)[sl] - th_b[sl], (ref["theta"] - th_b)[sl])
    finally:
        seld_lib.seld_v2_plan_destroy(plan)


# ------------------------------------------------------------------------------------------------ 7. seld_v2_swa
@pytest.mark.parametrize("n", [1, 255, 257, 4097])
def test_m_swa(seld_lib, n):
    rng = np.random.default_rng(n)
    stream = torch.cuda.Stream()
    for cnt in (0, 1, 2):
        swa, w = CT.f32(rng.standard_normal(n)), CT.f32(rng.standard_normal(n) * 3)
        buf = torch.full((n + 128,), float("nan"), device="cuda")
        buf[64:64 + n] = dev(swa)
        wd = dev(w)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            assert seld_lib.seld_v2_swa(ptr(buf[64:]), ptr(wd), n, cnt, _sp(stream)) == 0
        stream.synchronize()
        want = w if cnt == 0 else K.swa_numpy(swa, w, cnt)
        assert same(buf[64:64 + n].cpu().numpy(), want), cnt
        assert bool(torch.isnan(buf[:64]).all()) and bool(torch.isnan(buf[64 + n:]).all()) and same(wd.cpu().numpy(), w)


# ------------------------------------------------------------------------------------------------ 8. seld_aug_v2
def _aug_input(shape, seed):
    rng = np.random.default_rng(seed)
    x = CT.f32(rng.standard_normal(shape))
    x.reshape(-1)[rng.choice(x.size, 16, replace=False)] = -0.0      # a zero's sign survives where nothing is masked
    return x


def _banded(x, lead):
    """x inside a sentinel-filled allocation, `lead` floats from its (256-byte aligned) start -> (whole, view)"""
    whole = torch.full((lead + x.size + 64,), 7.25, device="cuda")
    view = whole[lead:lead + x.size].view(*x.shape)
    view.copy_(dev(x))
    return whole, view


@pytest.mark.parametrize("shape,lead", [((2, 200, 8, 7), 64), ((1, 100, 5, 10), 64), ((2, 200, 8, 7), 63)],
                         ids=["56-floats-16-byte", "50-floats-scalar", "56-floats-unaligned-scalar"])
def test_aug_v2(seld_lib, shape, lead):
    from seld_amd import transforms
    B, T, F, Cc = shape
    period, n_t, n_f = 100, 10, 6
    nseg = T // period
    x = _aug_input(shape, seed=T + F)
    shift, tm, fm = K.aug_draws(B, nseg, F, period, n_t, n_f, seed=3)
    assert np.abs(shift).min() > 0
    cases = {"all": (shift, tm, fm), "no time masks": (shift, None, fm), "no frequency masks": (shift, tm, None), "no shift": (None, tm, fm),
             "shift alone": (shift, None, None)}
    for name, (sh, t, f) in cases.items():
        want = K.aug_v2_numpy(x, sh, 4, t, f, period)
        whole, view = _banded(x, lead)
        if name == "shift alone":
            transforms.random_ups_and_downs(view, draws=sh)
        elif sh is None:      # the C entry point with shift = NULL (the tables in pinned memory, as transforms passes them)
            tabs = [torch.as_tensor(np.stack([m[1], m[0]])).pin_memory() for m in (t, f)]
            rc = seld_lib.seld_aug_v2(ptr(view), B, T, F, Cc, period, None, 4, ptr(tabs[0][0]), ptr(tabs[0][1]), n_t, ptr(tabs[1][0]), ptr(tabs[1][1]),
                                      n_f, C.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert rc == 0
        else:
            time = (6, n_t) if t is not None else (6, 0)
            freq = (8, n_f) if f is not None else (8, 0)
            empty = (np.zeros((0, B * nseg), np.int32),) * 2
            transforms.v2_sample_transforms(view, draws=(sh, t or empty, f or empty), time=time, freq=freq, period=period)
        torch.cuda.synchronize()
        got = view.cpu().numpy()
        assert np.array_equal(bits(got), bits(want)), name
        if t is not None:
            assert (bits(got[0, 40:48]) == 0).all(), name      # the two overlapping runs: +0.0, whatever stood there
        assert bool((whole[:lead] == 7.25).all()) and bool((whole[lead + x.size:] == 7.25).all()), name
        # what no run and no shifted channel covers holds its bits
        keep = bits(want) == bits(x)
        assert keep[..., 4:].any() and np.array_equal(bits(got)[keep], bits(x)[keep])
        if sh is not None:
            assert not np.array_equal(bits(got[..., :4]), bits(x[..., :4]))
        # the existing path: the add, then one transforms.mask per mask with the same draws, in the reference's order
        old = dev(x)
        if sh is not None:
            old[..., :4] += dev(sh).view(B, 1, 1, 1)
        for axis, m in ((-3, t), (-2, f)):
            for k in range(0 if m is None else m[0].shape[0]):
                transforms.mask(old, axis, period=period, draws=(m[0][k], m[1][k]))
        assert np.array_equal(bits(old.cpu().numpy()), bits(got)), name + ": the add + transforms.mask path"


# ------------------------------------------------------------------------------------------------ 9, 10. a full v2 step
def _check_update(name, w0, w1, ref_w1, tol=1e-4):
    """tests/test_trainv2_gpu.py::_check_update restated: theta_after - theta_before against the oracle's update; the update is only
    observable through the float32 weight it was added to, whose storage rounds by up to half an ulp, 2^-24 max|w|"""
    got, ref = w1.astype(np.float64) - w0, ref_w1 - w0
    err, bar = np.abs(got - ref).max(), tol * np.abs(ref).max() + 2.0 ** -24 * np.abs(w0).max()
    print(f"[parity] {name:40s} max |update - ref| = {err:.3e}  bar {bar:.3e}  (|update|max={np.abs(ref).max():.3e})")
    assert np.isfinite(w1).all() and err <= bar, (name, err, bar)


def _autograd_step(forward, tr, nt, w, st, x, ys, yd, wc, sed_loss, ls):
    """forward + trainv2_oracle.losses_v2 under autograd (no regulariser term: reg_agc_adabelief adds its gradient)"""
    from oracle import seldnet_oracle as O
    fw = V.t64(w).clone().requires_grad_(True)
    sed, doa, new_st = forward(O.unflatten(fw, tr), O.unflatten(V.t64(st), nt), V.t64(x))
    obj, sl, dl = V.losses_v2(sed, doa, V.t64(ys), V.t64(yd), V.t64(wc), sed_loss=sed_loss, loss_weights=(1.0, 1000.0), ls=ls)
    (g,) = torch.autograd.grad(obj, fw)
    return {"sed": sed.detach().numpy(), "doa": doa.detach().numpy(), "sloss": sl.detach().numpy(), "dloss": dl.detach().numpy(), "grad": g.numpy(),
            "new_state": torch.cat([new_st[n].detach().reshape(-1) for n, _ in nt]).numpy()}


@functools.lru_cache(maxsize=None)
def _ss5_ref(sed_loss, ls, nb):
    cfg, shape = CT.SS5_SMALL, CT.SS5_SMALL_INPUT
    tr, nt = CT.variable_specs(cfg, shape)
    w, st = CT.random_weights(cfg, shape, seed=11)
    x, ys, yd = CT.synthetic_batch(cfg, shape, seed=23)
    wc = CT.f32(np.random.default_rng(4).uniform(0.3, 3.0, cfg["n_classes"]))
    x, ys, yd = x[:nb], ys[:nb], yd[:nb]
    ref = _autograd_step(lambda wd, sd, xt: CT.forward(cfg, wd, sd, xt, True), tr, nt, w, st, x, ys, yd, wc, sed_loss, ls)
    return w, st, x, ys, yd, wc, ref


def _v2_step_check(tag, build, w, st, x, ys, yd, wc, ref, sed_loss, ls, l2=1e-3, through_trainv2=True):
    from seld_amd import losses, trainv2
    sel = losses.BinaryCrossentropy() if sed_loss == "BCE" else losses.focal_loss
    model = build()
    model.set_weights(w, st)
    assert trainv2.apply_kernel_regularizer(model, l2) is model
    cfg = trainv2._v2_cfg(sel, (1.0, 1000.0), ls, wc)
    opt = trainv2.AdaBelief(1e-3)
    y_p, sl, dl = model._v2_fwd_bwd(x, (ys, yd), cfg)
    got = {"sed": y_p[0].cpu().numpy(), "doa": y_p[1].cpu().numpy(), "sloss": sl.cpu().numpy(), "dloss": dl.cpu().numpy(), "g_raw": model.get_grads()}
    for k in ("sed", "doa", "sloss", "dloss"):
        check(f"{tag} {k}", got[k], ref[k])
    biggest = np.abs(ref["grad"]).max()
    for n, off, sh in model.variables:
        k = int(np.prod(sh))
        _check_or_zero(f"{tag} grad {n}", got["g_raw"][off:off + k], ref["grad"][off:off + k], biggest)
    check(f"{tag} BN state", model.get_weights()[1], ref["new_state"])
    # the optimizer stage against the oracle's stage applied to the library's own raw gradient: a first AdaBelief step is discontinuous in
    # the gradient (the update is lr sign(g) / 0.9), and so is the clip where a decision flips
    model._v2_opt(opt, l2, trainv2.CLIP_FACTOR)
    assert model.adam_step == 1
    shapes = [sh for _, _, sh in model.variables]
    reg = [int(trainv2.is_regularized_composed(n)) for n, _, _ in model.variables]
    assert 0 < sum(reg) < len(reg)
    o = V.reg_agc_adabelief(w, got["g_raw"], np.zeros_like(w), np.zeros_like(w), shapes, reg, 1, lr=1e-3, l2=l2, clip_factor=trainv2.CLIP_FACTOR)
    print(f"[parity] {tag}: {int((o['ratio'] >= 1).sum())} of {o['ratio'].size} units clipped")
    assert (o["ratio"] >= 1).any() and (o["ratio"] < 1).any()
    g1, (w1, st1) = model.get_grads(), model.get_weights()
    m1, v1 = model.rt.adam_m[:model.n_params].cpu().numpy(), model.rt.adam_v[:model.n_params].cpu().numpy()
    for n, off, sh in model.variables:
        s_ = slice(off, off + int(np.prod(sh)))
        check(f"{tag} consumed grad {n}", g1[s_], o["g"][s_])
        check(f"{tag} m {n}", m1[s_], o["m"][s_])
        check(f"{tag} v {n}", v1[s_], o["v"][s_])
        _check_update(f"{tag} update {n}", w[s_], w1[s_], o["theta"][s_])
    model.close()
    if not through_trainv2:
        return
    # the same step through seld_amd.trainv2 on a fresh model: identical bits
    model = build()
    model.set_weights(w, st)
    trainv2.apply_kernel_regularizer(model, l2)
    step = trainv2.generate_trainstep(sel, losses.MMSE_with_cls_weights, (1, 1000), label_smoothing=ls, cls_weights=wc)
    y2, sl2, dl2 = step(model, x, (ys, yd), trainv2.AdaBelief(1e-3))
    w2, st2 = model.get_weights()
    for name, a, b in (("sed", y2[0].cpu().numpy(), got["sed"]), ("doa", y2[1].cpu().numpy(), got["doa"]), ("sloss", sl2.cpu().numpy(), got["sloss"]),
                       ("dloss", dl2.cpu().numpy(), got["dloss"]), ("grad", model.get_grads(), g1), ("weights", w2, w1), ("state", st2, st1)):
        assert same(a, b), f"{tag} through trainv2: {name}"
    model.close()


@pytest.mark.parametrize("sed_loss,ls,nb", [("BCE", 0.1, 2), ("focal", 0.0, 2), ("BCE", 0.1, 1)], ids=["BCE-ls0.1", "focal", "batch-of-B-1"])
def test_full_v2_step_on_conv_temporal(sed_loss, ls, nb):
    """the "ss5" case of conv_temporal_oracle at (2, 52, 15, 7), every Dropout 0, explicit class weights; the last case runs a batch of
    B - 1 on the model built for B"""
    from seld_amd import losses, models, train
    w, st, x, ys, yd, wc, ref = _ss5_ref(sed_loss, ls, nb)
    build = lambda: models.conv_temporal(CT.SS5_SMALL_INPUT, copy.deepcopy(CT.SS5_SMALL))
    _v2_step_check(f"v2 conv_temporal {sed_loss} B={nb}", build, w, st, x, ys, yd, wc, ref, sed_loss, ls)
    if nb == 2 and sed_loss == "BCE":
        model = build()
        with pytest.raises(ValueError, match="composed models"):      # AGC inside train.trainstep stays refused for composed models
            train.trainstep(model, x, (ys, yd), losses.BinaryCrossentropy(), losses.MMSE, (1.0, 1000.0), train.Adam(1e-3), agc=True)
        model.close()


def _composed_seldnet_config(seldnet_config):
    cfg = copy.deepcopy(seldnet_config)
    cfg["FIRST"] = "mother_block"
    cfg["FIRST_ARGS"] = {"filters0": 8, "filters1": 12, "filters2": 0, "kernel_size0": 3, "kernel_size1": 3, "kernel_size2": 0, "connect0": [1],
                         "connect1": [0, 1], "connect2": [1, 0, 1], "strides": [5, 4], "activation": "relu"}
    return cfg


def test_full_v2_step_on_a_composed_seldnet(seldnet_config):
    """models.seldnet with a small mother_block FIRST and the bidirectional_GRU_block SECOND (modules.ComposedSeldNet)"""
    from oracle import modules_oracle as M
    from oracle import seldnet_oracle as O
    from seld_amd import models, modules
    cfg = _composed_seldnet_config(seldnet_config)
    shape = (2, 50, 16, 7)
    tr, nt = M.variable_specs(cfg, shape)
    w, st = M.random_weights(cfg, shape, seed=11)
    x, ys, yd = O.synthetic_batch(shape[0], shape[1], shape[2], shape[3], seed=23)
    wc = CT.f32(np.random.default_rng(4).uniform(0.3, 3.0, 12))
    ref = _autograd_step(lambda wd, sd, xt: M.forward(cfg, wd, sd, xt, True), tr, nt, w, st, x, ys, yd, wc, "BCE", 0.1)

    def build():
        m = models.seldnet(shape, copy.deepcopy(cfg))
        assert type(m) is modules.ComposedSeldNet and [(n, s) for n, _, s in m.variables] == tr
        return m
    _v2_step_check("v2 composed seldnet", build, w, st, x, ys, yd, wc, ref, "BCE", 0.1)


# ------------------------------------------------------------------------------------------------ 11. SWA
def test_swa_on_a_composed_model():
    from seld_amd import models, trainv2
    cfg, shape = CT.CHAIN2, CT.CHAIN2_INPUT
    model = models.conv_temporal(shape, copy.deepcopy(cfg))
    assert model.swa_count == 0
    with pytest.raises(ValueError):
        model.swa_apply()
    swa = trainv2.SWA(model, start_epoch=3, swa_freq=2)
    ref_w = ref_s = None
    fired = []
    for epoch in range(8):
        w, st = CT.random_weights(cfg, shape, seed=10 + epoch)
        model.set_weights(w, st)
        before = swa.cnt
        swa.on_epoch_end(epoch)
        if swa.cnt != before:
            fired.append(epoch)
            ref_w, ref_s = (w, st) if before == 0 else (V.swa_update(ref_w, w, before), V.swa_update(ref_s, st, before))
    assert fired == [e for e in range(8) if V.swa_fires(e, 3, 2)] == [2, 4, 6] and swa.cnt == model.swa_count == 3
    swa.on_train_end()
    w1, st1 = model.get_weights()
    assert model.n_state > 0 and same(w1, ref_w) and same(st1, ref_s)
    model.close()


# ------------------------------------------------------------------------------------------------ 12. the test step
def test_v2_teststep_on_a_composed_model():
    from seld_amd import losses, models, train, trainv2
    cfg, shape = CT.CHAIN2, CT.CHAIN2_INPUT
    w, st = CT.random_weights(cfg, shape, seed=11)
    x, ys, yd = CT.synthetic_batch(cfg, shape, seed=23)
    model = models.conv_temporal(shape, copy.deepcopy(cfg))
    model.set_weights(w, st)
    ts = trainv2.generate_teststep(losses.BinaryCrossentropy(), losses.MMSE_with_cls_weights)
    a = ts(model, x, (ys, yd))
    a = [a[0][0].cpu().numpy(), a[0][1].cpu().numpy(), a[1].cpu().numpy(), a[2].cpu().numpy()]
    b = train.teststep(model, x, (ys, yd), losses.BinaryCrossentropy(), losses.MMSE)
    b = [b[0][0].cpu().numpy(), b[0][1].cpu().numpy(), b[1].cpu().numpy(), b[2].cpu().numpy()]
    for u, v in zip(a, b):
        assert same(u, v)
    sed, doa = CT.inference(cfg, shape, w, st, x)
    check("v2 teststep sed", a[0], sed)
    check("v2 teststep doa", a[1], doa)
    assert same(model.get_weights()[0], w) and same(model.get_weights()[1], st)
    model.close()


# ------------------------------------------------------------------------------------------------ 13. isolation
def test_fused_v2_step_untouched_by_a_composed_v2_step(seldnet_config):
    from oracle import seldnet_oracle as O
    from seld_amd import losses, models, trainv2
    B, T = 2, 50
    spec = O.Spec.from_config(seldnet_config)
    w, st = O.random_weights(spec, 0)
    x, ys, yd = O.synthetic_batch(B, T)
    mk = lambda: trainv2.generate_trainstep(losses.focal_loss, losses.MMSE_with_cls_weights, (1, 1000), 0.1)

    def fused_step():
        model = models.seldnet((B, T, 64, 7), copy.deepcopy(seldnet_config))
        model.set_weights(w, st)
        trainv2.apply_kernel_regularizer(model, 1e-3)
        y_p, sl, dl = mk()(model, x, (ys, yd), trainv2.AdaBelief())
        out = [y_p[0].cpu().numpy(), y_p[1].cpu().numpy(), sl.cpu().numpy(), dl.cpu().numpy(), model.get_grads(), *model.get_weights()]
        del model
        return out

    first = fused_step()
    cfg, shape = CT.CHAIN2, CT.CHAIN2_INPUT
    other = models.conv_temporal(shape, copy.deepcopy(cfg))
    cx, cys, cyd = CT.synthetic_batch(cfg, shape, seed=23)
    trainv2.apply_kernel_regularizer(other, 1e-3)
    step = trainv2.generate_trainstep(losses.BinaryCrossentropy(), losses.MMSE_with_cls_weights, (1, 1000), 0.1, cls_weights=np.ones(5, np.float32))
    y_p, sl, dl = step(other, cx, (cys, cyd), trainv2.AdaBelief())
    assert bool(torch.isfinite(y_p[0]).all()) and np.isfinite(other.get_weights()[0]).all() and other.adam_step == 1
    trainv2.SWA(other, 1).on_epoch_end(0)
    second = fused_step()          # `other` is still alive
    for a, b in zip(first, second):
        assert same(a, b)
    other.close()
