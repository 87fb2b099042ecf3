"""Times the front convolution of models.conv_temporal two ways at the workload shape — x [32, 300, 64, 7], k = 7, 32 filters (SS5.json) —
and the whole SS5.json train step at B = 32:

  stem     modules.StemConv2D on the stem kernels: seld_stem_conv_fwd, seld_stem_conv_wgrad (seld_amd/csrc/stem.hip; no im2col buffer)
  im2col   the existing modules.Conv2D: seld_m_im2col + seld_m_gemm forward, seld_m_gemm_tn for the kernel / bias gradients (dx=None)

The comparison base is the im2col composition.  Both layers hold the same weights and see the same x and dz; HIP events around each single
call, the two paths alternating, median of --calls calls after 5 warm-up rounds.  The train step: train.trainstep (BCE + MSE, Adam) on
tests/golden/SS5.json verbatim (its Dropout draws included), HIP events around each step, median of --steps steps -> clips/s; recorded
with no target (there is nothing to compare it with).  Prints one JSON line; --out writes it to a file as well.  Needs a HIP device.

    python tools/bench_conv_temporal.py [--calls 30] [--steps 10] [--out profiles/conv_temporal_stem.json]

--recipe v2 measures the trainv2 recipe in place of the stem comparison: the SS5.json step through
trainv2.generate_trainstep (class-weighted BCE with label smoothing + MMSE_with_cls_weights, L2 regulariser, AGC, AdaBelief) next to the
Adam step above, the two alternating in one session; the kernels the optimizer stage launches; and seld_aug_v2 on the workload batch with
the reference's masks (6, 10) / (8, 6) next to the add + 16 transforms.mask calls it replaces, with the same draws.

    python tools/bench_conv_temporal.py --recipe v2 --calls 100 --steps 100 --out profiles/trainv2_composed.json
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

B, T, FQ, CH, K, F = 32, 300, 64, 7, 7, 32


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(v):
    q = lambda f: sorted(v)[int(f * (len(v) - 1))]
    return {"median": round(statistics.median(v), 4), "p10": round(q(0.1), 4), "p90": round(q(0.9), 4)}


def recipe_v2(a):
    from seld_amd import losses, models, train, trainv2, transforms
    out = {"device": torch.cuda.get_device_name(0), "shape": [B, T, FQ, CH], "calls": a.calls, "steps": a.steps}
    rng = np.random.default_rng(0)
    dev = torch.device("cuda", torch.cuda.current_device())
    x = torch.as_tensor(rng.standard_normal((B, T, FQ, CH), dtype=np.float32)).to(dev)
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "SS5.json")))
    ms = {}
    model = {k: models.conv_temporal((B, T, FQ, CH), cfg) for k in ("adam", "v2")}
    nc = model["v2"].n_classes
    S = model["v2"].S
    ys = (rng.random((B, S, nc)) < 0.1).astype(np.float32)
    yd = (rng.standard_normal((B, S, 3 * nc)) * np.tile(ys, 3)).astype(np.float32)
    y = (torch.as_tensor(ys).to(dev), torch.as_tensor(yd).to(dev))
    trainv2.apply_kernel_regularizer(model["v2"], 1e-3)
    v2 = trainv2.generate_trainstep(losses.BinaryCrossentropy(), losses.MMSE_with_cls_weights, (1, 1000), label_smoothing=0.1)
    adam, belief = train.Adam(1e-3), trainv2.AdaBelief(1e-3)
    steps = {"adam": lambda: train.trainstep(model["adam"], x, y, losses.BinaryCrossentropy(), losses.MSE, (1.0, 1000.0), adam),
             "v2": lambda: v2(model["v2"], x, y, belief)}
    ts = {k: [] for k in steps}
    for i in range(a.steps + 3):
        for k in steps:
            t = timed(steps[k])
            if i >= 3:
                ts[k].append(t)
    for k in steps:
        out[f"ss5_{k}_step"] = {"batch": B, "ms": stats(ts[k]), "clips_per_s": round(B / (statistics.median(ts[k]) * 1e-3), 1)}
    out["v2_over_adam"] = round(statistics.median(ts["v2"]) / statistics.median(ts["adam"]), 4)
    # the optimizer stage alone, and the kernels it launches
    m = model["v2"]
    out["v2_opt_ms"] = stats([timed(lambda: m._v2_opt(belief, 1e-3, trainv2.CLIP_FACTOR)) for _ in range(a.calls)])
    out["adam_opt_ms"] = stats([timed(lambda: m.rt.ck(m.lib.seld_m_adam(m.rt.p(m.rt.params), m.rt.p(m.rt.grads), m.rt.p(m.rt.adam_m), m.rt.p(m.rt.adam_v),
                                                                           m.n_params, 1e-3, 0.9, 0.999, 1e-7, 1, m.rt.st()))) for _ in range(a.calls)])
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            m._v2_opt(belief, 1e-3, trainv2.CLIP_FACTOR)
            torch.cuda.synchronize()
        out["v2_opt_kernels"] = [e.name for e in prof.events() if "kernel" in e.name.lower() and "launch" not in e.name.lower()]
    except Exception as e:      # no tracer on this box
        out["v2_opt_kernels"] = f"not traced ({type(e).__name__})"
    out["v2_opt_launches"] = len(out["v2_opt_kernels"]) if isinstance(out["v2_opt_kernels"], list) else None
    out["params"] = m.n_params
    for mm in model.values():
        mm.close()
    # seld_aug_v2 next to what it replaces, same draws; each call restores nothing: masking an already masked batch moves the same bytes
    nseg = T // 100
    draws = transforms.draw_v2(np.random.default_rng(1), B, nseg, FQ)
    xa, xb = x.clone(), x.clone()

    def old():
        xb[..., :4] += shift_dev.view(B, 1, 1, 1)
        for axis, mk in ((-3, draws[1]), (-2, draws[2])):
            for k in range(mk[0].shape[0]):
                transforms.mask(xb, axis, period=100, draws=(mk[0][k], mk[1][k]))

    shift_dev = torch.as_tensor(draws[0]).to(dev)
    ta, tb = [], []
    for i in range(a.calls + 5):
        t0 = timed(lambda: transforms.v2_sample_transforms(xa, draws=draws))
        t1 = timed(old)
        if i >= 5:
            ta.append(t0)
            tb.append(t1)
    ya, yb = x.clone(), x.clone()
    transforms.v2_sample_transforms(ya, draws=draws)
    xb = yb
    old()
    torch.cuda.synchronize()
    out["aug_v2"] = {"ms": stats(ta), "add_plus_16_masks_ms": stats(tb), "speedup": round(statistics.median(tb) / statistics.median(ta), 2),
                     "same_bits": bool(torch.equal(ya.view(torch.int32), yb.view(torch.int32))), "batch_mb": round(x.numel() * 4 / 1e6, 1)}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as o:
            o.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--recipe", choices=("v1", "v2"), default="v1", help="v2: the trainv2 recipe's step and seld_aug_v2 in place of the stem comparison")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_conv_temporal needs a HIP device: nothing is measured without one")
    if a.recipe == "v2":
        return recipe_v2(a)
    from seld_amd import losses, models, modules, train
    out = {"device": torch.cuda.get_device_name(0), "shape": [B, T, FQ, CH], "k": K, "filters": F, "calls": a.calls}
    rng = np.random.default_rng(0)
    dev = torch.device("cuda", torch.cuda.current_device())
    x = torch.as_tensor(rng.standard_normal((B, T, FQ, CH), dtype=np.float32)).to(dev)
    dz = torch.as_tensor(rng.standard_normal((B, T, FQ, F), dtype=np.float32)).to(dev)
    # ---- the two layers, each on a runtime of its own, with the same weights
    rts, layers = {}, {}
    for name in ("stem", "im2col"):
        rt = modules._Rt(dev)
        layers[name] = (modules.StemConv2D(rt, "c", (T, FQ, CH), F, K, B, direct={"fwd": True, "wgrad": True}) if name == "stem"
                        else modules.Conv2D(rt, "c", (T, FQ, CH), F, K, (1, 1), B))
        rt.finalize()
        rts[name] = rt
    w = torch.as_tensor(rng.standard_normal(rts["stem"].n_params).astype(np.float32) * 0.05).to(dev)
    for rt in rts.values():
        rt.params[:rt.n_params].copy_(w)
    fwd = {"stem": lambda: layers["stem"].forward(x, B), "im2col": lambda: layers["im2col"].forward(x, B)}
    bwd = {"stem": lambda: layers["stem"].backward(dz, B), "im2col": lambda: layers["im2col"].backward(dz, None, B, 0)}
    times = {f"{p}_{n}": [] for p in ("fwd", "wgrad") for n in ("stem", "im2col")}
    for i in range(a.calls + 5):
        for n in ("stem", "im2col"):
            t = timed(fwd[n])
            if i >= 5:
                times[f"fwd_{n}"].append(t)
        for n in ("stem", "im2col"):
            t = timed(bwd[n])
            if i >= 5:
                times[f"wgrad_{n}"].append(t)
    zs = [layers[n].z[:B * T * FQ].reshape(-1) for n in ("stem", "im2col")]
    gs = [rts[n].grads[:rts[n].n_params] for n in ("stem", "im2col")]
    out["agreement"] = {"z": float((zs[0] - zs[1]).abs().max() / zs[1].abs().max()), "grads": float((gs[0] - gs[1]).abs().max() / gs[1].abs().max())}
    out["ms"] = {k: stats(v) for k, v in times.items()}
    out["im2col_over_stem"] = {p: round(out["ms"][f"{p}_im2col"]["median"] / out["ms"][f"{p}_stem"]["median"], 3) for p in ("fwd", "wgrad")}
    out["im2col_buffer_mb"] = round(B * T * FQ * K * K * CH * 4 / 1e6, 1)
    out["StemConv2D_DIRECT"] = dict(modules.StemConv2D.DIRECT)
    del layers, rts, fwd, bwd
    torch.cuda.empty_cache()
    # ---- the whole SS5.json train step
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "SS5.json")))
    model = models.conv_temporal((B, T, FQ, CH), cfg)
    nc = model.n_classes
    ys = (rng.random((B, model.S, nc)) < 0.1).astype(np.float32)
    yd = (rng.standard_normal((B, model.S, 3 * nc)) * np.tile(ys, 3)).astype(np.float32)
    ysd, ydd = torch.as_tensor(ys).to(dev), torch.as_tensor(yd).to(dev)
    opt = train.Adam(1e-3)
    step = lambda: train.trainstep(model, x, (ysd, ydd), losses.BinaryCrossentropy(), losses.MSE, (1.0, 1000.0), opt)
    ts = []
    for i in range(a.steps + 3):
        t = timed(step)
        if i >= 3:
            ts.append(t)
    out["ss5_train_step"] = {"batch": B, "steps": a.steps, "ms": stats(ts), "clips_per_s": round(B / (statistics.median(ts) * 1e-3), 1),
                             "params": model.n_params}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as o:
            o.write(line + "\n")


if __name__ == "__main__":
    main()
