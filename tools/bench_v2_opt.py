"""Times the optimizer stage alone on a seldnet.json and a resnet50_gru.json context: train.py's seld_adam_step(agc=1) (one agc_kernel launch
per variable + adam_kernel) against trainv2's seld_v2_opt_step(l2=1e-3, clip_factor=0.01) (two launches), DESIGN.md section 3i.  One real
seld_train_fwd_bwd fills the gradient buffer; before every timed call weights, gradients and moments are restored outside the event pair, so
both paths see the same data every time.  HIP events around each single call, the two paths alternating, median of --calls calls.  Prints one
JSON line.  --trace-calls N: N calls of each path and nothing else, for a rocprofv3 --kernel-trace --stats run of its own (launch counts).
Needs a HIP device.

    python tools/bench_v2_opt.py [--calls 200] [--trace-calls 0]
"""
import argparse
import copy
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

SELDNET = {
    "FIRST": "simple_conv_block", "FIRST_ARGS": {"filters": [64, 64, 64], "pool_size": [[5, 4], [1, 4], [1, 2]], "dropout_rate": 0.0},
    "SECOND": "bidirectional_GRU_block", "SECOND_ARGS": {"units": [128, 128], "dropout_rate": 0.0},
    "SED": "simple_dense_block", "SED_ARGS": {"units": [128], "n_classes": 14, "activation": "sigmoid", "name": "sed_out"},
    "DOA": "simple_dense_block", "DOA_ARGS": {"units": [128], "n_classes": 42, "activation": "tanh", "name": "doa_out"}, "n_classes": 12}


def configs():
    rn = copy.deepcopy(SELDNET)
    rn["FIRST"], rn["FIRST_ARGS"] = "resnet50_block", {"filters": 32, "block_num": [3, 4, 6, 3]}
    return {"seldnet": SELDNET, "resnet50_gru": rn}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--trace-calls", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_v2_opt needs a HIP device: nothing is measured without one")
    from seld_amd import _lib, losses, models, train, trainv2
    out = {"calls": a.calls, "device": torch.cuda.get_device_name(0)}
    B, T = 2, 100
    rng = np.random.default_rng(0)
    for name, cfg in configs().items():
        model = models.seldnet((B, T, 64, 7), cfg)
        x = rng.standard_normal((B, T, 64, 7), dtype=np.float32)
        ys = (rng.random((B, T // 5, 12)) < 0.1).astype(np.float32)
        yd = (rng.standard_normal((B, T // 5, 36)) * np.tile(ys, 3)).astype(np.float32)
        xd = model._prep(x)
        ysd, ydd = train._labels(model, (ys, yd), B)
        lc = train._cfg(losses.MMSE, (1.0, 1000.0))
        _lib.check(model.lib.seld_train_fwd_bwd(model.ctx, xd.data_ptr(), ysd.data_ptr(), ydd.data_ptr(), C.byref(lc), None, None, None, None), model.ctx)
        trainv2.apply_kernel_regularizer(model, 1e-3)
        torch.cuda.synchronize()
        gt, pt = model.grad_tensor(), model.param_tensor()
        g0, p0 = gt.clone(), pt.clone()
        zeros = np.zeros(model.n_params, np.float32)

        def restore():
            gt.copy_(g0)
            pt.copy_(p0)

        old = lambda: _lib.check(model.lib.seld_adam_step(model.ctx, 1e-3, 0.9, 0.999, 1e-7, 1), model.ctx)
        new = lambda: _lib.check(model.lib.seld_v2_opt_step(model.ctx, 1e-3, 0.9, 0.999, 1e-7, 1e-3, 0.01), model.ctx)
        if a.trace_calls:
            for _ in range(a.trace_calls):
                restore(); old(); restore(); new()
            torch.cuda.synchronize()
            continue
        times = {"adam_agc": [], "v2_opt": []}
        for i in range(a.calls + 10):
            for key, fn in (("adam_agc", old), ("v2_opt", new)):
                restore()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                if i >= 10:      # 10 warm-up rounds
                    times[key].append(e0.elapsed_time(e1))
        q = lambda v, f: sorted(v)[int(f * (len(v) - 1))]
        out[name] = {"variables": len(model.variables), "params": model.n_params, "launches": {"adam_agc": len(model.variables) + 1, "v2_opt": 2},
                     **{f"{k}_ms": {"median": round(statistics.median(v), 5), "p10": round(q(v, 0.1), 5), "p90": round(q(v, 0.9), 5)} for k, v in times.items()}}
        _lib.check(model.lib.seld_set_adam_host(model.ctx, zeros.ctypes.data, zeros.ctypes.data, model.n_params, 0), model.ctx)
        del model
    print(json.dumps(out))


if __name__ == "__main__":
    main()
