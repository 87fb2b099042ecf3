"""Times the recurrent-dropout entries seld_rnn_lstm_drop_fwd / _bwd (seld_amd/csrc/lstm.hip) and seld_rnn_gru_drop_fwd / _bwd (gru.hip) against
their non-dropout entries seld_rnn_lstm_fwd / _bwd and seld_rnn_gru_fwd / _bwd in the same process at B = 32, S = 600, both directions, every
forward in its saving (training) form.  The protocol of tools/bench_rnn.py: HIP events around 20 back-to-back calls after 5 warm-up calls,
median of 5 windows.  The non-dropout entry is timed twice, before and after the dropout one, so the run reports its own run-to-run spread:
`spread` = |a - b| / mean(a, b), `ratio` = dropout / mean(a, b).  Prints one JSON line and writes it to --out.  Needs a HIP device.

    python tools/bench_rnn_dropout.py [--shape 32,600] [--rate 0.2] [--out profiles/rnn_dropout.json]
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
    ap.add_argument("--shape", default="32,600")
    ap.add_argument("--rate", type=float, default=0.2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rnn_dropout.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rnn_dropout needs a HIP device: nothing is measured without one")
    from seld_amd import _lib
    lib = _lib.load()
    B, S = (int(v) for v in a.shape.split(","))
    R = B * S
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    pp = lambda ts: (p(ts[0]), p(ts[1]))
    g = torch.Generator(device="cpu").manual_seed(0)
    rn = lambda *sh: torch.randn(*sh, generator=g).cuda()
    two = lambda *sh: [torch.empty(*sh).cuda() for _ in (0, 1)]
    rm = [((torch.rand(B, 128, generator=g) >= a.rate).float() / (1.0 - a.rate)).cuda() for _ in (0, 1)]
    res = {}
    for kind, G in (("gru", 384), ("lstm", 512)):
        # recurrent kernels of half tools/bench_rnn.py's scale: Keras multiplies the masked state by 1 / (1 - rate) at every step, and with the
        # full scale the GRU state diverges on long sequences (not finite by S = 2400); the time does not depend on the values
        gx, U, dh = [rn(R, G) for _ in (0, 1)], [0.5 * rn(128, G) / math.sqrt(128) for _ in (0, 1)], [rn(R, 128) for _ in (0, 1)]
        brec = [0.1 * rn(G) for _ in (0, 1)]
        h, hm, c, sv, dgx, dgh = two(R, 128), two(R, 128), two(R, 128), two(R, 512), two(R, G), two(R, G)
        if kind == "gru":
            calls = {"fwd": (lambda: lib.seld_rnn_gru_fwd(*pp(gx), *pp(U), *pp(brec), *pp(h), *pp(sv), B, S, 128, st),
                             lambda: lib.seld_rnn_gru_drop_fwd(*pp(gx), *pp(U), *pp(brec), *pp(rm), *pp(h), *pp(hm), *pp(sv), B, S, 128, st)),
                     "bwd": (lambda: lib.seld_rnn_gru_bwd(*pp(dh), *pp(h), *pp(sv), *pp(U), *pp(dgx), *pp(dgh), B, S, 128, st),
                             lambda: lib.seld_rnn_gru_drop_bwd(*pp(dh), *pp(hm), *pp(sv), *pp(U), *pp(rm), *pp(dgx), *pp(dgh), B, S, 128, st))}
        else:
            calls = {"fwd": (lambda: lib.seld_rnn_lstm_fwd(*pp(gx), *pp(U), *pp(h), *pp(c), *pp(sv), B, S, 128, st),
                             lambda: lib.seld_rnn_lstm_drop_fwd(*pp(gx), *pp(U), *pp(rm), *pp(h), *pp(c), *pp(sv), B, S, 128, st)),
                     "bwd": (lambda: lib.seld_rnn_lstm_bwd(*pp(dh), *pp(c), *pp(sv), *pp(U), *pp(dgx), B, S, 128, st),
                             lambda: lib.seld_rnn_lstm_drop_bwd(*pp(dh), *pp(c), *pp(sv), *pp(U), *pp(rm), *pp(dgx), B, S, 128, st))}

        def run(fn):
            assert fn() == 0

        for pas in ("fwd", "bwd"):      # the forward first: the backward reads what the (dropout) forward left
            plain, drop = calls[pas]
            t0 = timed(lambda: run(plain))
            td = timed(lambda: run(drop))
            t1 = timed(lambda: run(plain))
            run(drop)
            mean = 0.5 * (t0 + t1)
            res[f"{kind}_{pas}"] = {"plain_ms": [round(t0, 4), round(t1, 4)], "drop_ms": round(td, 4), "spread": round(abs(t0 - t1) / mean, 4),
                                    "ratio": round(td / mean, 4), "drop_us_per_step": round(1e3 * td / S, 3)}
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(x).all()) for x in h + dgx)
    out = {"B": B, "S": S, "directions": 2, "rate": a.rate, **res, "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
