"""Times the any-width attention seld_attnw_fwd + seld_attnw_bwd (seld_amd/csrc/attention.hip) for every key_dim of
nas_seldnet.search_space_1d_attention at S = 60, 300 and 600 frames (B = 32 clips, H = 4 heads, the forward in its saving form), and, for
the widths that are no multiple of 8, seld_attn_fwd + _bwd at the padded width 8 ceil(d / 8) on caller-padded operands in the same run: the
call the ragged form replaces, which it must not be slower than — it runs the same MFMA chains and moves fewer floats.  The protocol of
tools/bench_relattn.py: HIP events around 20 back-to-back calls after 5 warm-up calls, median of 5 windows.  seld_attn_* at d = 24, S = 300
is timed twice, before and after the sweep, so the run reports its own run-to-run spread; `slower_than_padded` lists the ragged cases whose
forward + backward exceeds the padded call's by more than that spread.  Prints one JSON line and writes it to --out.  Needs a HIP device.

    python tools/bench_attn_width.py [--shape 32,4] [--lengths 60 300 600] [--out profiles/attn_width.json]
"""
import argparse
import ctypes as C
import json
import math
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_relattn import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="32,4", help="B,H")
    ap.add_argument("--lengths", nargs="*", type=int, default=[60, 300, 600])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_width.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attn_width needs a HIP device: nothing is measured without one")
    from seld_amd import _lib, nas_seldnet
    lib = _lib.load()
    B, H = (int(v) for v in a.shape.split(","))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    g = torch.Generator(device="cpu").manual_seed(0)

    def measure(S, d, width, fwd, bwd, scratch_fn):
        """heads of d real columns inside `width` (d: the ragged call; 8 ceil(d / 8): zero-padded for the narrow entries)"""
        R, HD = B * S, H * width
        def operand():
            t = torch.zeros(R, H, width)
            t[:, :, :d] = torch.randn(R, H, d, generator=g)
            return t.reshape(R, HD).cuda()
        q, k, v, do = (operand() for _ in range(4))
        o, dq, dk, dv = (torch.empty(R, HD).cuda() for _ in range(4))
        lse = torch.empty(B * H * S).cuda()
        scratch = torch.empty(int(scratch_fn(B, S, H, width))).cuda()
        scale = 1.0 / math.sqrt(d)

        def f():
            assert fwd(p(q), p(k), p(v), HD, HD, HD, p(o), p(lse), B, S, H, width, scale, st) == 0

        def b():
            assert bwd(p(q), p(k), p(v), HD, HD, HD, p(o), p(do), p(lse), p(dq), p(dk), p(dv), HD, HD, HD, p(scratch), B, S, H, width, scale, st) == 0
        tf = timed(f)      # the forward first: the backward reads what it left
        tb = timed(b)
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(x).all()) for x in (o, dq, dk, dv))
        return {"fwd_ms": round(tf, 4), "bwd_ms": round(tb, 4), "ms": round(tf + tb, 4)}

    narrow = (lib.seld_attn_fwd, lib.seld_attn_bwd, lib.seld_attn_bwd_scratch)
    wide = (lib.seld_attnw_fwd, lib.seld_attnw_bwd, lib.seld_attnw_bwd_scratch)
    anchor = [measure(300, 24, 24, *narrow)]
    cases = {}
    for S in a.lengths:
        for d in nas_seldnet.search_space_1d_attention["transformer_encoder_stage"]["key_dim"]:
            row = {"attnw": measure(S, d, d, *wide)}
            if d % 8:
                dp = 8 * ((d + 7) // 8)
                row["padded_width"] = dp
                row["attn_padded"] = measure(S, d, dp, *narrow)
                row["ratio"] = round(row["attnw"]["ms"] / row["attn_padded"]["ms"], 4)
            cases[f"S{S} d{d}"] = row
    anchor.append(measure(300, 24, 24, *narrow))
    spread = round(abs(anchor[0]["ms"] - anchor[1]["ms"]) / (0.5 * (anchor[0]["ms"] + anchor[1]["ms"])), 4)
    slower = sorted(k for k, r in cases.items() if "ratio" in r and r["ratio"] > 1.0 + spread)
    out = {"B": B, "H": H, "lengths": a.lengths, "anchor_attn_d24_S300": anchor, "spread": spread, "cases": cases,
           "slower_than_padded": slower, "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
