"""Times one conformer_encoder_stage (seld_amd/modules.py) and its two depthwise kernels (seld_amd/csrc/conformer.hip) with device events:
the stage's forward and forward + backward, and seld_dwconv1d_fwd / _bwd alone next to the bytes the algorithm has to move
(forward: read [R, 2D], write [R, D]; backward: read u and dy, write du).  Prints one JSON line.  Needs a HIP device.

    python tools/bench_conformer.py [--batch 32] [--frames 600] [--width 128] [--kernel 32] [--steps 50] [--warmup 10]
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

HBM_PEAK = 8.0e12      # bytes / s, the MI355X's nominal HBM3E rate


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--width", type=int, default=128)
    ap.add_argument("--kernel", type=int, default=32)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_conformer needs a HIP device: nothing is measured without one")
    from seld_amd import modules
    B, S, D, k = a.batch, a.frames, a.width, a.kernel
    cfg = {"depth": 1, "n_head": 4, "key_dim": 32, "kernel_size": k, "multiplier": 4, "dropout_rate": 0, "pos_encoding": "basic"}
    stage = modules.conformer_encoder_stage(cfg)((B, S, D))
    rt = stage.blocks[0].rt
    rt.finalize()
    g = torch.Generator(device="cpu").manual_seed(0)
    rt.params[:rt.n_params].copy_(0.05 * torch.randn(rt.n_params, generator=g))
    rt.state[:rt.n_state].fill_(1.0)
    R = B * S
    x, dy = torch.randn(R, D, generator=g).cuda(), torch.randn(R, D, generator=g).cuda()
    fwd = timed(lambda: stage.forward(x, B, True), a.steps, a.warmup)
    both = timed(lambda: (stage.forward(x, B, True), stage.backward(dy, B)), a.steps, a.warmup)
    # the two kernels alone
    lib, st = rt.lib, rt.st()
    p = lambda t: C.c_void_p(t.data_ptr())
    u, w, bias, y = torch.randn(R, 2 * D, generator=g).cuda(), torch.randn(k, D, generator=g).cuda(), torch.zeros(D).cuda(), torch.empty(R, D).cuda()
    du, dw, db = torch.empty(R, 2 * D).cuda(), torch.empty(k, D).cuda(), torch.empty(D).cuda()
    scratch = torch.empty(int(lib.seld_dwconv1d_bwd_scratch(B, S, D, k))).cuda()

    def kf():
        rc = lib.seld_dwconv1d_fwd(p(u), 2 * D, p(w), p(bias), p(y), B, S, D, k, 1, st)
        assert rc == 0

    def kb():
        rc = lib.seld_dwconv1d_bwd(p(u), 2 * D, p(w), p(dy), p(du), 2 * D, p(dw), p(db), p(scratch), B, S, D, k, 1, st)
        assert rc == 0

    t_f, t_b = timed(kf, a.steps, a.warmup), timed(kb, a.steps, a.warmup)
    bytes_f, bytes_b = 4 * R * 3 * D, 4 * R * 5 * D
    print(json.dumps({"shape": {"B": B, "S": S, "D": D, "k": k}, "stage_fwd_ms": round(fwd, 4), "stage_fwd_bwd_ms": round(both, 4),
                      "dwconv_fwd_ms": round(t_f, 5), "dwconv_fwd_MB": round(bytes_f / 1e6, 2),
                      "dwconv_fwd_hbm_fraction": round(bytes_f / (t_f * 1e-3) / HBM_PEAK, 4),
                      "dwconv_bwd_ms": round(t_b, 5), "dwconv_bwd_MB": round(bytes_b / 1e6, 2),
                      "dwconv_bwd_hbm_fraction": round(bytes_b / (t_b * 1e-3) / HBM_PEAK, 4), "hbm_peak_bytes_per_s": HBM_PEAK}))


if __name__ == "__main__":
    main()
