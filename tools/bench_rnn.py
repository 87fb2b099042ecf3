"""Times seld_rnn_lstm_fwd / _bwd (seld_amd/csrc/lstm.hip) against seld_m_gru_fwd / _bwd (gru.hip) in the same process at B = 32, S = 600 (the shape of
the GRU record), both directions, the forward pass in its saving (training) form.  HIP events around 20 back-to-back calls after
5 warm-up calls, median of 5 windows: the protocol of tools/bench_relattn.py.  Prints one JSON line.  Needs a HIP device.

    python tools/bench_rnn.py [--shape 32,600]
"""
import argparse
import ctypes as C
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_relattn import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="32,600")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rnn needs a HIP device: nothing is measured without one")
    from seld_amd import _lib
    lib = _lib.load()
    B, S = (int(v) for v in a.shape.split(","))
    R = B * S
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    g = torch.Generator(device="cpu").manual_seed(0)
    rn = lambda *sh: torch.randn(*sh, generator=g).cuda()
    two = lambda *sh: [torch.empty(*sh).cuda() for _ in (0, 1)]
    t = {}
    for kind, G in (("gru", 384), ("lstm", 512)):
        gx, U, dh = [rn(R, G) for _ in (0, 1)], [rn(128, G) / math.sqrt(128) for _ in (0, 1)], [rn(R, 128) for _ in (0, 1)]
        brec = [0.1 * rn(G) for _ in (0, 1)]
        h, c, sv, dgx, dgh = two(R, 128), two(R, 128), two(R, 512), two(R, G), two(R, G)
        pp = lambda ts: (p(ts[0]), p(ts[1]))
        if kind == "gru":
            fwd = lambda: lib.seld_m_gru_fwd(*pp(gx), *pp(U), *pp(brec), *pp(h), *pp(sv), None, B, S, 128, st)
            bwd = lambda: lib.seld_m_gru_bwd(p(dh[0]), *pp(h), *pp(sv), *pp(U), *pp(dgx), *pp(dgh), B, S, 128, st)
        else:
            fwd = lambda: lib.seld_rnn_lstm_fwd(*pp(gx), *pp(U), *pp(h), *pp(c), *pp(sv), B, S, 128, st)
            bwd = lambda: lib.seld_rnn_lstm_bwd(*pp(dh), *pp(c), *pp(sv), *pp(U), *pp(dgx), B, S, 128, st)

        def run(fn):
            assert fn() == 0

        t[f"{kind}_fwd_ms"] = timed(lambda: run(fwd))
        t[f"{kind}_bwd_ms"] = timed(lambda: run(bwd))
        assert all(bool(torch.isfinite(x).all()) for x in h + dgx)
    out = {"B": B, "S": S, "directions": 2, **{k: round(v, 4) for k, v in t.items()},
           "fwd_us_per_step": {k: round(1e3 * t[f"{k}_fwd_ms"] / S, 3) for k in ("gru", "lstm")},
           "bwd_us_per_step": {k: round(1e3 * t[f"{k}_bwd_ms"] / S, 3) for k in ("gru", "lstm")},
           "lstm_over_gru_fwd": round(t["lstm_fwd_ms"] / t["gru_fwd_ms"], 3), "lstm_over_gru_bwd": round(t["lstm_bwd_ms"] / t["gru_bwd_ms"], 3),
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
