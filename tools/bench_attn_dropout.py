"""Times seld_attn_drop_fwd / _bwd at rate 0.1 against seld_attn_fwd / _bwd of the same build (seld_amd/csrc/attention.hip) at the shapes of
tests/test_attention_gpu.py::test_attention_bench_shape: what the probability masks' Philox calls cost.  The two
versions of a call alternate window by window in one process (what else runs on the host then falls on both alike): HIP events around
`--steps` back-to-back calls after `--warmup` calls of each, `--windows` windows each; median, and the spread of the windows.  Prints one JSON
line.  Needs a HIP device.  Under a kernel profiler, `--steps 5 --windows 1` gives the three kernels' times per instantiation.

    python tools/bench_attn_dropout.py [--shapes 32,600,4,24 32,600,4,48] [--rate 0.1]
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def window(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def timed_pair(plain, drop, steps, warmup, windows):
    """-> (ms per call of each: median of the windows, and each one's (min, max))"""
    for fn in (plain, drop):
        for _ in range(warmup):
            fn()
    a, b = [], []
    for _ in range(windows):
        a.append(window(plain, steps))
        b.append(window(drop, steps))
    return statistics.median(a), statistics.median(b), (min(a), max(a)), (min(b), max(b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=["32,600,4,24", "32,600,4,48"])
    ap.add_argument("--rate", type=float, default=0.1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--windows", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attn_dropout needs a HIP device: nothing is measured without one")
    from seld_amd import _lib
    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    g = torch.Generator(device="cpu").manual_seed(0)
    seed, layer, step = 0x5e1d5e1d5e1d5e1d, 4098, 1
    rows = []
    for shape in a.shapes:
        B, S, H, d = (int(v) for v in shape.split(","))
        R, HD, scale = B * S, H * d, 1.0 / math.sqrt(d)
        q, k, v, do = (torch.randn(R, HD, generator=g).cuda() for _ in range(4))
        o, od, lse = torch.empty(R, HD).cuda(), torch.empty(R, HD).cuda(), torch.empty(B * H * S).cuda()
        dq, dk, dv = (torch.empty(R, HD).cuda() for _ in range(3))
        scratch = torch.empty(int(lib.seld_attn_bwd_scratch(B, S, H, d))).cuda()

        def fwd():
            assert lib.seld_attn_fwd(p(q), p(k), p(v), HD, HD, HD, p(o), p(lse), B, S, H, d, scale, st) == 0

        def fwd_drop():
            assert lib.seld_attn_drop_fwd(p(q), p(k), p(v), HD, HD, HD, p(od), p(lse), B, S, H, d, scale, a.rate, seed, layer, step, st) == 0

        def bwd():
            assert lib.seld_attn_bwd(p(q), p(k), p(v), HD, HD, HD, p(o), p(do), p(lse), p(dq), p(dk), p(dv), HD, HD, HD, p(scratch), B, S, H, d,
                                     scale, st) == 0

        def bwd_drop():
            assert lib.seld_attn_drop_bwd(p(q), p(k), p(v), HD, HD, HD, p(od), p(do), p(lse), p(dq), p(dk), p(dv), HD, HD, HD, p(scratch), B, S, H, d,
                                          scale, a.rate, seed, layer, step, st) == 0

        f0, f1, fs0, fs1 = timed_pair(fwd, fwd_drop, a.steps, a.warmup, a.windows)      # (leaves o, od and lse for the backward calls)
        b0, b1, bs0, bs1 = timed_pair(bwd, bwd_drop, a.steps, a.warmup, a.windows)
        r4 = lambda x: round(x, 4)
        rows.append({"B": B, "S": S, "H": H, "d": d, "rate": a.rate, "attn_fwd_ms": r4(f0), "attn_drop_fwd_ms": r4(f1), "fwd_ratio": round(f1 / f0, 3),
                     "attn_bwd_ms": r4(b0), "attn_drop_bwd_ms": r4(b1), "bwd_ratio": round(b1 / b0, 3),
                     "window_min_max_ms": {"attn_fwd": [r4(x) for x in fs0], "attn_drop_fwd": [r4(x) for x in fs1], "attn_bwd": [r4(x) for x in bs0],
                                           "attn_drop_bwd": [r4(x) for x in bs1]}})
    print(json.dumps({"kernels": rows, "steps": a.steps, "windows": a.windows}))


if __name__ == "__main__":
    main()
