"""Times the any-width GRU recurrence seld_rnn_gruw_fwd / _bwd (seld_amd/csrc/gru_w.hip) at the architecture search's shape — B = 256 clips
(nas_seldnet's batch), S = 60 steps, both directions, the forward in its saving (training) form — for every GRU width of
nas_seldnet.search_space_1d, and, at 128 units, the shipped seld_rnn_gru_fwd / _bwd (gru.hip) on the same inputs in the same run: the figure
a generic-width kernel is set against.  The protocol of tools/bench_rnn.py: HIP events around 20 back-to-back calls after 5 warm-up calls,
median of 5 windows.  The shipped kernel is timed twice, before and after the sweep, so the run reports its own run-to-run spread.  Per
width: the plan (form, clips per workgroup), ms per call, microseconds per step, and the recurrent product's arithmetic rate (2 * 3u^2 FLOP
per clip, direction and step forward; the same backward).  Prints one JSON line and writes it to --out.  Needs a HIP device.

    python tools/bench_gru_width.py [--shape 256,60] [--out profiles/gru_width.json]
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
    ap.add_argument("--shape", default="256,60")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gru_width.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gru_width needs a HIP device: nothing is measured without one")
    from seld_amd import _lib, nas_seldnet
    lib = _lib.load()
    B, S = (int(v) for v in a.shape.split(","))
    R = B * S
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    pp = lambda ts: (p(ts[0]), p(ts[1]))
    g = torch.Generator(device="cpu").manual_seed(0)
    rn = lambda *sh: torch.randn(*sh, generator=g).cuda()
    two = lambda *sh: [torch.empty(*sh).cuda() for _ in (0, 1)]

    def measure(u, fwd, bwd):
        gx, U, dh = [rn(R, 3 * u) for _ in (0, 1)], [rn(u, 3 * u) / math.sqrt(u) for _ in (0, 1)], [rn(R, u) for _ in (0, 1)]
        brec = [0.1 * rn(3 * u) for _ in (0, 1)]
        h, sv, dgx, dgh = two(R, u), two(R, 4 * u), two(R, 3 * u), two(R, 3 * u)

        def f():
            assert fwd(*pp(gx), *pp(U), *pp(brec), *pp(h), *pp(sv), B, S, u, st) == 0

        def b():
            assert bwd(*pp(dh), *pp(h), *pp(sv), *pp(U), *pp(dgx), *pp(dgh), B, S, u, st) == 0
        tf = timed(f)      # the forward first: the backward reads what it left
        tb = timed(b)
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(x).all()) for x in h + dgx + dgh)
        flop = 2.0 * 3 * u * u * B * 2 * S
        return {"fwd_ms": round(tf, 4), "bwd_ms": round(tb, 4), "fwd_us_per_step": round(1e3 * tf / S, 3), "bwd_us_per_step": round(1e3 * tb / S, 3),
                "fwd_gflops": round(flop / tf * 1e-6, 1), "bwd_gflops": round(flop / tb * 1e-6, 1)}

    shipped = [measure(128, lib.seld_rnn_gru_fwd, lib.seld_rnn_gru_bwd)]
    widths = {}
    plan = (C.c_int32 * 4)()
    for u in nas_seldnet.search_space_1d["bidirectional_GRU_stage"]["units"]:
        lib.seld_rnn_gruw_plan(u, plan)
        widths[str(u)] = dict({"form": int(plan[0]), "clips_per_workgroup": int(plan[1])}, **measure(u, lib.seld_rnn_gruw_fwd, lib.seld_rnn_gruw_bwd))
    shipped.append(measure(128, lib.seld_rnn_gru_fwd, lib.seld_rnn_gru_bwd))
    spread = {k: round(abs(shipped[0][k] - shipped[1][k]) / (0.5 * (shipped[0][k] + shipped[1][k])), 4) for k in ("fwd_ms", "bwd_ms")}
    out = {"B": B, "S": S, "directions": 2, "shipped_128": shipped, "shipped_spread": spread, "gruw": widths,
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
