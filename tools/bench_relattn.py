"""Times seld_relattn_fwd / _bwd (seld_amd/csrc/relattn.hip) and, in the same process, seld_attn_fwd / _bwd (attention.hip) at the shapes of
DESIGN.md section 3e, and one attention_block (seld_amd/modules.py) forward and forward + backward.  HIP events around 20 back-to-back calls
after 5 warm-up calls, median of 5 windows: the protocol of section 3e.  Prints one JSON line.  Needs a HIP device.

    python tools/bench_relattn.py [--shapes 32,600,4,24 32,600,4,48] [--block 32,600,192]
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


def timed(fn, steps=20, warmup=5, windows=5):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / steps)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=["32,600,4,24", "32,600,4,48"])
    ap.add_argument("--block", default="32,600,192")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_relattn needs a HIP device: nothing is measured without one")
    from seld_amd import _lib, modules
    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    g = torch.Generator(device="cpu").manual_seed(0)
    rows = []
    for shape in a.shapes:
        B, S, H, d = (int(v) for v in shape.split(","))
        R, HD, scale = B * S, H * d, 1.0 / math.sqrt(d)
        q, k, v, do = (torch.randn(R, HD, generator=g).cuda() for _ in range(4))
        P, u, vb = torch.randn(S, HD, generator=g).cuda(), torch.randn(HD, generator=g).cuda(), torch.randn(HD, generator=g).cuda()
        o, lse = torch.empty(R, HD).cuda(), torch.empty(B * H * S).cuda()
        dqu, dqv, dk, dv, dP = tuple(torch.empty(R, HD).cuda() for _ in range(4)) + (torch.empty(S, HD).cuda(),)
        s_rel = torch.empty(int(lib.seld_relattn_bwd_scratch(B, S, H, d))).cuda()
        s_att = torch.empty(int(lib.seld_attn_bwd_scratch(B, S, H, d))).cuda()

        def rel_f():
            assert lib.seld_relattn_fwd(p(q), p(k), p(v), HD, HD, HD, p(P), HD, p(u), p(vb), p(o), p(lse), B, S, H, d, scale, st) == 0

        def rel_b():
            assert lib.seld_relattn_bwd(p(q), p(k), p(v), HD, HD, HD, p(P), HD, p(u), p(vb), p(o), p(do), p(lse), p(dqu), p(dqv), p(dk), p(dv), p(dP),
                                        HD, HD, HD, HD, HD, p(s_rel), B, S, H, d, scale, st) == 0

        def att_f():
            assert lib.seld_attn_fwd(p(q), p(k), p(v), HD, HD, HD, p(o), p(lse), B, S, H, d, scale, st) == 0

        def att_b():
            assert lib.seld_attn_bwd(p(q), p(k), p(v), HD, HD, HD, p(o), p(do), p(lse), p(dqu), p(dk), p(dv), HD, HD, HD, p(s_att), B, S, H, d, scale,
                                     st) == 0

        t = {"attn_fwd_ms": timed(att_f), "attn_bwd_ms": timed(att_b)}
        att_f()
        t.update({"relattn_fwd_ms": timed(rel_f), "relattn_bwd_ms": timed(rel_b)})
        rows.append(dict({"B": B, "S": S, "H": H, "d": d}, **{n: round(x, 4) for n, x in t.items()},
                         fwd_ratio=round(t["relattn_fwd_ms"] / t["attn_fwd_ms"], 2), bwd_ratio=round(t["relattn_bwd_ms"] / t["attn_bwd_ms"], 2)))
    B, S, D = (int(v) for v in a.block.split(","))
    cfg = {"key_dim": 48, "n_head": 4, "kernel_size": 3, "ff_kernel_size": 1, "ff_multiplier": 2, "ff_factor0": 0.5, "ff_factor1": 0.5,
           "use_glu": True, "dropout_rate": 0}
    stage = modules.attention_block(cfg)((B, S, D))
    rt = stage.blocks[0].rt
    rt.finalize()
    rt.params[:rt.n_params].copy_(0.05 * torch.randn(rt.n_params, generator=g))
    rt.state[:rt.n_state].fill_(1.0)
    x, dy = torch.randn(B * S, D, generator=g).cuda(), torch.randn(B * S, D, generator=g).cuda()
    fwd = timed(lambda: stage.forward(x, B, True))
    both = timed(lambda: (stage.forward(x, B, True), stage.backward(dy, B)))
    print(json.dumps({"kernels": rows, "attention_block": {"B": B, "S": S, "D": D, "config": cfg, "fwd_ms": round(fwd, 4), "fwd_bwd_ms": round(both, 4)}}))


if __name__ == "__main__":
    main()
