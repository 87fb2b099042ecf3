"""Times models.spectro_temporal_attention_based_VAD at the reference's training shape — B = 256 windows of [7, 80, 1], default config
(train_vad_baseline.py:110-114) — and its gated spectral tail two ways at each of the four stage shapes:

  fused      seld_vad_gate_pool_fwd + _bwd (seld_amd/csrc/vad.hip): a * sigmoid(b) and MaxPooling2D([1, 2]) in one pass each way
  composed   the operators the library had before: seld_m_act (sigmoid), seld_rnn_merge_fwd (mul), seld_pool2d_fwd; seld_pool2d_bwd,
             seld_rnn_merge_bwd (mul), seld_m_act_bwd — the gated tensor, sigmoid(b) and their gradients in memory

Both run as vad._GatedStage runs them (tail_forward + tail_backward with the argmax bytes), on the same BatchNormalization outputs of a real
forward and the same dy.  A sample is HIP events on the stream around --reps forward + backward pairs (a pair takes some 20
microseconds: one pair would time the launches); the two paths alternate; median of --calls samples after 5 warm-up rounds.  The fused form is
the default (vad.SpectroTemporalVAD.FUSED_GATE) only if its sum over the four stages is below the composition's in the same run: the result
records both sums and `fused_wins`.  Then the whole train step (BCE of the three outputs, Adam; and AdaBelief as train_vad_baseline.py:47)
and inference: HIP events around each call, median of --steps after 3 warm-up calls.  Prints one JSON line; --out writes it to a file as well.
Needs a HIP device.

    python tools/bench_vad.py [--calls 30] [--reps 20] [--steps 20] [--out profiles/vad.json]
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
CFG = {"dropout_rate": 0.0}


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_vad needs a HIP device: nothing is measured without one")
    from seld_amd import train, trainv2, vad
    dev = torch.device("cuda", torch.cuda.current_device())
    rng = np.random.default_rng(0)
    x = torch.as_tensor(rng.standard_normal((B,) + SHAPE, dtype=np.float32)).to(dev)
    y = torch.as_tensor((rng.random((B, SHAPE[0])) < 0.5).astype(np.float32)).to(dev)
    out = {"device": torch.cuda.get_device_name(0), "input": [B] + list(SHAPE), "config": dict(vad.CONFIG_DEFAULTS, **CFG), "calls": a.calls,
           "reps": a.reps, "steps": a.steps}
    models = {"fused": vad.SpectroTemporalVAD((B,) + SHAPE, CFG, fused_gate=True), "composed": vad.SpectroTemporalVAD((B,) + SHAPE, CFG, fused_gate=False)}
    w, st = models["fused"].get_weights()
    models["composed"].set_weights(w, st)
    for m in models.values():      # one real training forward fills every stage's BatchNormalization outputs
        m(x, training=True)
    torch.cuda.synchronize()
    # ---- the gated tail, stage by stage
    stages, sums = [], {"fused": 0.0, "composed": 0.0}
    for i in range(len(models["fused"].stages)):
        sf, sc = models["fused"].stages[i], models["composed"].stages[i]
        sc.ya.copy_(sf.ya)
        sc.yb.copy_(sf.yb)
        dy = torch.as_tensor(rng.standard_normal((B,) + sf.out_shape, dtype=np.float32)).to(dev)
        runs = {n: (lambda s=s: (s.tail_forward(B, True), s.tail_backward(dy, B))) for n, s in (("fused", sf), ("composed", sc))}
        ts = {n: [] for n in runs}
        for r in range(a.calls + 5):
            for n in runs:
                t = timed(runs[n], a.reps)
                if r >= 5:
                    ts[n].append(t)
        rel = lambda p, q: float((p - q).abs().max() / q.abs().max())
        rec = {"rows_W_C": [B * sf.T, sf.W, sf.C], "fused_ms": stats(ts["fused"]), "composed_ms": stats(ts["composed"]),
               "agreement": {"y": rel(sf.y, sc.y), "da": rel(sf.da, sc.da), "db": rel(sf.db, sc.db), "same_winners": bool(torch.equal(sf.idx, sc.idx))}}
        n_el = B * sf.T * sf.W * sf.C
        # bytes the fused pair must move: forward reads a, b, writes y and the argmax bytes; backward reads a, b, dy, the bytes, writes da, db
        rec["fused_bytes"] = int(4 * n_el * 6 + (n_el // sf.W) * (sf.W // 2) * (4 * 2 + 2))
        rec["fused_gb_per_s"] = round(rec["fused_bytes"] / (rec["fused_ms"]["median"] * 1e-3) / 1e9, 1)
        for n in sums:
            sums[n] += rec[f"{n}_ms"]["median"]
        stages.append(rec)
    out["gate_pool_fwd_bwd"] = {"stages": stages, "fused_sum_ms": round(sums["fused"], 5), "composed_sum_ms": round(sums["composed"], 5),
                                "composed_over_fused": round(sums["composed"] / sums["fused"], 3), "fused_wins": bool(sums["fused"] < sums["composed"]),
                                "FUSED_GATE": bool(vad.SpectroTemporalVAD.FUSED_GATE)}
    # ---- the whole step, both gate paths alternating, and inference
    adam, belief = train.Adam(1e-3), trainv2.AdaBelief(1e-4)
    calls = {"train_step_adam_fused": lambda: models["fused"].train_step(x, y, adam), "train_step_adam_composed": lambda: models["composed"].train_step(x, y, adam),
             "train_step_adabelief_fused": lambda: models["fused"].train_step(x, y, belief), "inference_fused": lambda: models["fused"](x),
             "inference_composed": lambda: models["composed"](x)}
    ts = {n: [] for n in calls}
    for r in range(a.steps + 3):
        for n in calls:
            t = timed(calls[n])
            if r >= 3:
                ts[n].append(t)
    for n in calls:
        out[n] = {"ms": stats(ts[n]), "windows_per_s": round(B / (statistics.median(ts[n]) * 1e-3), 1)}
    out["params"] = models["fused"].n_params
    for m in models.values():
        m.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as o:
            o.write(line + "\n")


if __name__ == "__main__":
    main()
