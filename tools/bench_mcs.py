"""Times seld_aug_mcs, the one-launch CGMM mask estimator behind transforms.mcs_aug (recorded with no target).

HIP events around --reps calls per shape after --warmup calls, on seeded randn input [B,T,F,C]:
  (32,300,64,7) iteration 2     a foa batch
  (32,300,64,7) iteration 10    the same with five times the rounds: the small-matrix section's share
  (32,300,64,10) iteration 2    a mic batch, the widest C
  (1,3000,64,7) iteration 2     one whole clip: the most frames a column holds
  (1,300,64,7) iteration 2      its pair: 64 columns again, one per CU, a tenth of the frames; the difference is the per-frame work
Beside each: the traffic floor, one read and one write of x at 6.3 TB/s (what HBM3E sustains of its 8 TB/s peak), and the ratio.  For scale, the
wall time of the literal float64 oracle (tests/mcs_oracle.py) on the CPU for the first shape.

python tools/bench_mcs.py [--reps 20] [--warmup 3] [--no-oracle]  -> one JSON line, also written to profiles/mcs_aug.json
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

HBM_BYTES_PER_S = 6.3e12
SHAPES = [((32, 300, 64, 7), 2), ((32, 300, 64, 7), 10), ((32, 300, 64, 10), 2), ((1, 3000, 64, 7), 2), ((1, 300, 64, 7), 2)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-oracle", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mcs_aug.json"))
    a = ap.parse_args()
    from seld_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("bench_mcs.py needs a HIP device: a time taken elsewhere says nothing")
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rows = []
    for shape, iteration in SHAPES:
        torch.manual_seed(0)
        x = torch.randn(shape).cuda()
        out = torch.empty_like(x)
        B, T, F, Cc = shape

        def call():
            rc = lib.seld_aug_mcs(C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), None, None, B, T, F, Cc, iteration, 1e-6, stream)
            assert rc == 0, rc
        for _ in range(a.warmup):
            call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        ms = np.array(ms)
        floor_ms = 2 * x.numel() * 4 / HBM_BYTES_PER_S * 1e3
        rows.append({"shape": list(shape), "iteration": iteration, "ms_median": float(np.median(ms)), "p10": float(np.percentile(ms, 10)),
                     "p90": float(np.percentile(ms, 90)), "traffic_floor_ms": floor_ms, "times_floor": float(np.median(ms) / floor_ms),
                     "finite": bool(torch.isfinite(out).all())})
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "hbm_bytes_per_s": HBM_BYTES_PER_S, "shapes": rows}
    if not a.no_oracle:
        import mcs_oracle
        shape, iteration = SHAPES[0]
        torch.manual_seed(0)
        xc = torch.randn(shape)
        t0 = time.perf_counter()
        mcs_oracle.mcs(xc, iteration)
        res["cpu_oracle_s"] = {"shape": list(shape), "iteration": iteration, "wall_s": time.perf_counter() - t0, "threads": torch.get_num_threads()}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
