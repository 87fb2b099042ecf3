"""Times models.vad_architecture at the search's training shape — B = 256 windows of [7, 80, 1] (nas_vad.py:26, 191-192) — on three fixed
configurations, each with the head two ways:

  fused      seld_vadarch_head_fwd + seld_vadarch_head_bwd (seld_amd/csrc/vadarch.hip): three kernels — the probabilities; the loss, dx and the
             chunks' partial dw, db; their sums
  composed   the operators the library had before, six calls: Linear (seld_m_gemm), seld_m_act, seld_vad_bce, seld_m_act_bwd, seld_m_gemm_tn,
             seld_m_gemm

  dense      flatten, simple_dense_stage 2 x 512 relu, last_unit 7 (models_test.py's configuration, Dropout at 0): the head is [256, 512] x 7
  mother     one mother_stage (3 x 3, 16 filters, strides (1, 2)), simple_dense_stage 1 x 64 relu, last_unit 1: the head is [1792, 64] x 1
  mother2    two mother_stages (8 and 16 filters) and the head on the 4-D tensor: [1792, 80 * 16] x 1

For each: the train step (Adam) of two models with the same weights, the two alternating — HIP events around --reps steps, median of --calls
samples after 5 warm-up rounds; the head's own launches alone, on the features of a real forward, the same way; the LIBRARY CALLS of one
step counted on the host — not kernel launches: a call is one or more of them.  The fused head's kernels are known from its source: three
(forward one, backward two); the composed head's six calls are at least seven kernels (seld_vad_bce is two, seld_m_gemm_tn a product and
its reduction) and were not counted from a trace.  There is no parent-commit number: the model is new, and the composed head of
the same commit is the baseline.  `fused_not_slower` holds where the fused step's median is not above the composed one's; VadArchNet's
fused_head=None may mean the fused head only while it holds for all three.  Prints one JSON line; --out writes it to a file as well.  Needs
a HIP device.

    python tools/bench_vadarch.py [--calls 30] [--reps 20] [--out profiles/vadarch.json]
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

B, SHAPE = 256, (7, 80, 1)
FUSED_HEAD_KERNELS = 3      # csrc/vadarch.hip: head_fwd_kernel; head_bwd_kernel, head_bwd_final_kernel


def _mother(filters, strides):
    return {"depth": 1, "filters0": 0, "filters1": filters, "filters2": 0, "kernel_size0": 0, "kernel_size1": 3, "kernel_size2": 0,
            "connect0": [1], "connect1": [0, 0], "connect2": [0, 0, 1], "strides": list(strides)}


CONFIGS = {
    "dense": {"flatten": True, "last_unit": 7, "BLOCK0": "simple_dense_stage",
              "BLOCK0_ARGS": {"depth": 2, "units": 512, "activation": "relu", "dropout_rate": 0.0}},
    "mother": {"flatten": False, "last_unit": 1, "BLOCK0": "mother_stage", "BLOCK0_ARGS": _mother(16, (1, 2)),
               "BLOCK1": "simple_dense_stage", "BLOCK1_ARGS": {"depth": 1, "units": 64, "activation": "relu", "dropout_rate": 0.0}},
    "mother2": {"flatten": False, "last_unit": 1, "BLOCK0": "mother_stage", "BLOCK0_ARGS": _mother(8, (1, 1)),
                "BLOCK1": "mother_stage", "BLOCK1_ARGS": _mother(16, (1, 1))},
}


def timed(fn, reps=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def stats(v):
    q = lambda f: sorted(v)[int(f * (len(v) - 1))]
    return {"median": round(statistics.median(v), 5), "p10": round(q(0.1), 5), "p90": round(q(0.9), 5)}


def alternate(runs, calls, reps):
    ts = {n: [] for n in runs}
    for r in range(calls + 5):
        for n in runs:
            t = timed(runs[n], reps)
            if r >= 5:
                ts[n].append(t)
    return {n: stats(v) for n, v in ts.items()}


def library_calls(fn):
    """the C-ABI calls (modules._Rt.ck -> _lib.check) of one fn()"""
    from seld_amd import _lib
    count, check = [0], _lib.check

    def counting(rc, ctx=None):
        count[0] += 1
        return check(rc, ctx)

    _lib.check = counting
    try:
        fn()
    finally:
        _lib.check = check
    return count[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_vadarch needs a HIP device: nothing is measured without one")
    from seld_amd import modules, train
    dev = torch.device("cuda", torch.cuda.current_device())
    rng = np.random.default_rng(0)
    x = torch.as_tensor(rng.standard_normal((B,) + SHAPE, dtype=np.float32)).to(dev)
    out = {"device": torch.cuda.get_device_name(0), "input": [B] + list(SHAPE), "calls": a.calls, "reps": a.reps, "configs": {}}
    rel = lambda p, q: float((p - q).abs().max() / q.abs().max())
    for name, cfg in CONFIGS.items():
        models = {"fused": modules.VadArchNet((B,) + SHAPE, cfg, fused_head=True), "composed": modules.VadArchNet((B,) + SHAPE, cfg, fused_head=False)}
        mf, mc = models["fused"], models["composed"]
        w, st = mf.get_weights()
        mc.set_weights(w, st)
        y = torch.as_tensor((rng.random(mf.output_shape()) < 0.5).astype(np.float32)).to(dev)
        R = B * mf.S
        rec = {"config": cfg, "head_rows_D_U": [R, mf.D, mf.last_unit], "params": mf.n_params, "macs_per_window": mf.complexity()["flops"]}
        # ---- one step each from the same weights: the two heads agree, and the calls of a step
        adam = train.Adam(0.0)
        rec["library_calls_per_step"] = {n: library_calls(lambda m=m: m.train_step(x, y, adam)) for n, m in models.items()}
        torch.cuda.synchronize()
        lf, lc = float(mf.train_step(x, y, adam)[1]), float(mc.train_step(x, y, adam)[1])
        rec["agreement"] = {"loss": abs(lf - lc) / abs(lc), "grads": rel(mf.rt.grads, mc.rt.grads)}
        # ---- the head alone, on the features of that forward
        runs = {n: (lambda m=m: m._loss(m._head_forward(m.feat, R).view(m.output_shape()), y, True)) for n, m in models.items()}
        rec["head_library_calls"] = {n: library_calls(runs[n]) for n in runs}
        rec["head_kernel_launches"] = {"fused": FUSED_HEAD_KERNELS, "composed": "at least 7; not traced"}
        rec["head_fwd_bwd_ms"] = alternate(runs, a.calls, a.reps)
        # bytes the fused head must move: x twice (forward, backward), dx once, p and y, w three times, the partial dw written and read
        D, U = mf.D, mf.last_unit
        nc = int(mf.rt.lib.seld_vadarch_head_bwd_scratch(R, D, U)) // (D * U + 1 + U)
        rec["fused_head_bytes"] = int(4 * (R * D * (2 if mf.on_data else 3) + 4 * R * U + 3 * D * U + 2 * nc * D * U))
        rec["fused_head_gb_per_s"] = round(rec["fused_head_bytes"] / (rec["head_fwd_bwd_ms"]["fused"]["median"] * 1e-3) / 1e9, 1)
        # ---- the whole train step
        adam = train.Adam(1e-3)
        steps = {n: (lambda m=m: m.train_step(x, y, adam)) for n, m in models.items()}
        rec["train_step_ms"] = alternate(steps, a.calls, a.reps)
        rec["windows_per_s"] = {n: round(B / (rec["train_step_ms"][n]["median"] * 1e-3), 1) for n in steps}
        rec["fused_not_slower"] = bool(rec["train_step_ms"]["fused"]["median"] <= rec["train_step_ms"]["composed"]["median"])
        out["configs"][name] = rec
        for m in models.values():
            m.close()
    out["fused_not_slower_on_all"] = all(r["fused_not_slower"] for r in out["configs"].values())
    out["FUSED_HEAD"] = bool(modules.VadArchNet.FUSED_HEAD)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as o:
            o.write(line + "\n")


if __name__ == "__main__":
    main()
