"""Times the front convolution of models.conv_temporal two ways at the workload shape — x [32, 300, 64, 7], k = 7, 32 filters (SS5.json) —
and the whole SS5.json train step at B = 32:

  stem     modules.StemConv2D on the stem kernels: seld_stem_conv_fwd, seld_stem_conv_wgrad (seld_amd/csrc/stem.hip; no im2col buffer)
  im2col   the existing modules.Conv2D: seld_m_im2col + seld_m_gemm forward, seld_m_gemm_tn for the kernel / bias gradients (dx=None)

The comparison base is the im2col composition.  Both layers hold the same weights and see the same x and dz; HIP events around each single
call, the two paths alternating, median of --calls calls after 5 warm-up rounds.  The train step: train.trainstep (BCE + MSE, Adam) on
tests/golden/SS5.json verbatim (its Dropout draws included), HIP events around each step, median of --steps steps -> clips/s; recorded
with no target (there is nothing to compare it with).  Prints one JSON line; --out writes it to a file as well.  Needs a HIP device.

    python tools/bench_conv_temporal.py [--calls 30] [--steps 10] [--out profiles/conv_temporal_stem.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_conv_temporal needs a HIP device: nothing is measured without one")
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
