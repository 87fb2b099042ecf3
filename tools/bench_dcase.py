"""Times the on-device DCASE scorer (recorded with no target).

  1. HIP events around SELDMetrics_.update_seld_scores + utils.answer_rows for --files files of 600 label frames and 12 classes
     (random activity and reference tracks, labels packed and uploaded beforehand);
  2. the wall time of one trainv2 evaluate_fn on one [3000, 64, 7] clip with the small SS5 configuration of the tests;
  3. HIP events around one SELDMetrics_.sweep_seld_scores (12 classes, search_best.BASE_THRESHOLD on a flat 0.5 table) on the files of 1.,
     and around the loop it replaces: the same 97 threshold vectors through update_seld_scores, one call each from a reset state, the
     states kept on the device and copied to the host once.  The two are timed alternately.

python tools/bench_dcase.py [--files 100] [--reps 20]  -> one JSON line
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def random_labels(rng, T, nc, K):
    d = {}
    for t0 in range(0, T, 10):
        for c in range(nc):
            if rng.random() < 0.5:
                for f in np.nonzero(rng.random(10) < 0.8)[0]:
                    for tid in rng.permutation(K + 2)[:rng.integers(1, K + 1)]:
                        v = rng.standard_normal(3)
                        d.setdefault(t0 + int(f), []).append([c, *(v / np.linalg.norm(v)), int(tid)])
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=100)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    from seld_amd import models, trainv2, utils
    from seld_amd.SELD_evaluation_metrics import SELDMetrics_
    from conv_temporal_oracle import SS5_SMALL
    rng = np.random.default_rng(0)
    T, nc, K = 600, 12, 2
    packed = utils.concat_labels([utils.pack_labels(random_labels(rng, T, nc, K), T, nc) for _ in range(a.files)])
    outs = [(torch.rand(T, nc, device="cuda"), torch.randn(T, 3 * nc, device="cuda")) for _ in range(a.files)]
    sed, doa = torch.cat([s for s, _ in outs]), torch.cat([d for _, d in outs])
    m = SELDMetrics_(nb_classes=nc)
    packed.to_device(m._dev)
    ms = []
    for _ in range(a.reps + 3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        m.update_seld_scores(outs, packed)
        utils.answer_rows(sed, doa, 0.5, packed.file_off)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms = np.array(ms[3:])
    clip = rng.standard_normal((3000, 64, 7)).astype(np.float32)
    model = models.conv_temporal((10, 300, 64, 7), dict(SS5_SMALL))
    fn = trainv2.generate_evaluate_fn([clip], [random_labels(rng, T, nc, K)], None, batch_size=32)
    fn(model, 0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(model, 1)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    from seld_amd import search_best
    cand = search_best.BASE_THRESHOLD
    vectors = []
    for c in range(nc):
        for v in cand:
            vectors.append(utils.thresh_table(0.5, nc))
            vectors[-1][c] = v
    vectors.append(utils.thresh_table(0.5, nc))

    def sweep():
        return m.sweep_seld_scores(outs, packed, 0.5, cand)

    def loop():
        states = []
        for v in vectors:
            m.reset_states()
            m.update_seld_scores(outs, packed, v)
            states.append(m.state.clone())
        return torch.stack(states).cpu().numpy()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out
    sw, lp = [], []
    for i in range(a.reps + 3):
        t_s, (table, base) = timed(sweep)
        t_l, states = timed(loop)
        sw.append(t_s)
        lp.append(t_l)
    same = bool(np.array_equal(np.concatenate([table.reshape(-1, 11), base[None]]).view(np.uint64), states.view(np.uint64)))
    sw, lp = np.array(sw[3:]), np.array(lp[3:])
    print(json.dumps({"files": a.files, "frames": T, "classes": nc, "reps": a.reps, "score_and_rows_ms_median": float(np.median(ms)),
                      "p10": float(np.percentile(ms, 10)), "p90": float(np.percentile(ms, 90)), "evaluate_fn_wall_s": wall,
                      "candidates": len(cand), "sweep_ms_median": float(np.median(sw)), "sweep_p10": float(np.percentile(sw, 10)),
                      "sweep_p90": float(np.percentile(sw, 90)), "loop97_ms_median": float(np.median(lp)),
                      "loop97_p10": float(np.percentile(lp, 10)), "loop97_p90": float(np.percentile(lp, 90)), "sweep_equals_loop_bits": same}))


if __name__ == "__main__":
    main()
