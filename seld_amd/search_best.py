"""The per-class SED threshold search that the reference's search_best.py names and never runs: its candidate grid
(`base_threshold`, search_best.py:145), its fold-5 / fold-6 label lists (:148-166) and its model average (:139-144) are there, the loop over
thresholds is commented out, and make_answer.py:156 carries a hand-made table (`[0.35, 0.35, 0.3, 0.4, 0.65, ...]`).  One evaluation there
is csv files, nested dicts and a Hungarian call per (frame, class).

Here one seld_dcase_sweep call (SELDMetrics_.sweep_seld_scores) returns the counters of every single-class change of the current table,
bit for bit what nc x M update_seld_scores calls would leave, and `search_thresholds` descends on them: take the (class, candidate) with the
lowest SELD score while it is strictly below the current one.  The walk is deterministic: ties go to the first (class, candidate) in
row-major order.

    python -m seld_amd.search_best --models SS5.json:a.npz SS5.json:b.npz --feat_path F --label_path L --ans_path METADATA_DEV/ \\
        --mode val --out thresholds.json [--write_answers DIR]"""
from __future__ import annotations

import numpy as np

from . import metrics as _metrics, utils
from .SELD_evaluation_metrics import seld_scores_from_state

BASE_THRESHOLD = (0.3, 0.35, 0.4, 0.45, 0.55, 0.6, 0.65, 0.7)      # search_best.py:145
MODES = {'val': ('dev-val', 5), 'test': ('dev-test', 6)}           # search_best.py:148-166: label folder, fold digit
MAX_CANDIDATES = 16                                                # SELD_DCASE_MAX_CAND
WIN_SIZE, STEP_SIZE = 300, 5                                       # ensemble_outputs' defaults (search_best.py:23-24)


def state_score(state) -> float:
    """the eleven counters -> metrics.calculate_seld_score of the four metrics"""
    return float(_metrics.calculate_seld_score(seld_scores_from_state(state)))


def choose_step(table, base):
    """table [nc, M, 11], base [11] (sweep_seld_scores) -> (c, k, score) of the lowest-scoring single-class change, the first one in
    row-major (c, k) order on a tie, or None unless that score is strictly below the base row's."""
    table = np.asarray(table, np.float64)
    nc, M = table.shape[:2]
    scores = np.array([[state_score(table[c, k]) for k in range(M)] for c in range(nc)], np.float64)
    flat = int(np.argmin(scores.reshape(-1)))          # the first minimum
    c, k = divmod(flat, M)
    if not scores[c, k] < state_score(base):
        return None
    return c, k, float(scores[c, k])


def _candidates(candidates) -> np.ndarray:
    cand = np.asarray(candidates, np.float32).reshape(-1)
    if not 1 <= cand.size <= MAX_CANDIDATES or not np.isfinite(cand).all():
        raise ValueError(f"search_thresholds takes 1..{MAX_CANDIDATES} finite candidates, got {cand.size}")
    return cand


def search_thresholds(pred, gt, candidates=BASE_THRESHOLD, start=0.5, doa_threshold=20, nb_classes=12, max_steps=None, device=None,
                      sweep=None):
    """Coordinate descent over per-class thresholds from thresh_table(start): one sweep, choose_step, thr[c] = candidates[k], until no
    single-class change lowers the score or `max_steps` (default nc * M) steps are taken.  The score falls strictly over a finite set of
    tables, so the loop ends.  `pred` / `gt` are what SELDMetrics_.update_seld_scores takes; `sweep`, a callable thr -> (table, base),
    replaces the device call (the loop then needs no device).
    -> (thresholds float32 [nc], score, (ER, F, LE, LR), steps [(c, k, score), ...])"""
    cand = _candidates(candidates)
    nc = int(nb_classes)
    thr = utils.thresh_table(start, nc).copy()
    if max_steps is None:
        max_steps = nc * cand.size
    if sweep is None:
        from .SELD_evaluation_metrics import SELDMetrics_
        scorer = SELDMetrics_(doa_threshold=doa_threshold, nb_classes=nc, device=device)
        if not isinstance(gt, utils.PackedLabels):
            gt = utils.concat_labels(gt)          # packed once, swept many times
        sweep = lambda t: scorer.sweep_seld_scores(pred, gt, t, cand)
    steps = []
    table, base = sweep(thr)
    while len(steps) < max_steps:
        step = choose_step(table, base)
        if step is None:
            break
        c, k, score = step
        thr[c] = cand[k]
        steps.append((int(c), int(k), float(score)))
        table, base = sweep(thr)
    return thr, state_score(base), seld_scores_from_state(base), steps


def _parse_models(entries):
    import os
    out = []
    for e in entries or ():
        cfg, sep, weights = str(e).partition(':')
        if not sep or not cfg or not weights:
            raise ValueError(f"--models takes cfg.json:weights.npz pairs, got {e!r}")
        for p in (cfg, weights):
            if not os.path.isfile(p):
                raise ValueError(f"--models {e!r}: no such file {p}")
        out.append((cfg, weights))
    if not out:
        raise ValueError("--models: at least one cfg.json:weights.npz pair")
    return out


def _labels(ans_path, mode):
    """the label files of `mode` as search_best.py:153-166 lists them -> (names, cartesian dicts)"""
    import os
    from glob import glob
    folder, fold = MODES[mode]
    files = [f for f in sorted(glob(os.path.join(ans_path, folder, '*'))) if os.path.basename(f)[4:5] == str(fold)]
    names = [os.path.splitext(os.path.basename(f))[0] for f in files]
    return names, [utils.convert_output_format_polar_to_cartesian(utils.load_output_format_file(f)) for f in files]


def main(argv=None):
    """Search the thresholds of a model average on fold 5 (`--mode val`) or fold 6 (`--mode test`) and write them, with the score and the
    four metrics before and after and the steps taken, to `--out`.  -> the dict written."""
    import argparse
    import json
    import os
    ap = argparse.ArgumentParser(prog="python -m seld_amd.search_best", description=__doc__.split("\n\n")[0])
    ap.add_argument("--models", nargs="+", required=True, metavar="CFG.json:WEIGHTS.npz")
    ap.add_argument("--feat_path", required=True)
    ap.add_argument("--label_path", required=True)
    ap.add_argument("--ans_path", required=True)
    ap.add_argument("--mode", default="val")
    ap.add_argument("--candidates", type=float, nargs="+", default=list(BASE_THRESHOLD))
    ap.add_argument("--start", type=float, default=0.5)
    ap.add_argument("--out", default="thresholds.json")
    ap.add_argument("--write_answers", default=None, metavar="DIR")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--doa_threshold", type=float, default=20)
    a = ap.parse_args(argv)
    # configuration errors first: none of them needs a device
    if a.mode not in MODES:
        raise ValueError(f"--mode must be one of {sorted(MODES)}, got {a.mode!r}")
    saved = _parse_models(a.models)
    cand = _candidates(a.candidates)
    if a.batch < 1:
        raise ValueError("--batch must be positive")
    from . import data_loader as dl
    xs, _ = dl.load_seldnet_data(a.feat_path, a.label_path, mode=a.mode)
    names, dicts = _labels(a.ans_path, a.mode)
    if not xs or len(xs) != len(dicts):
        raise ValueError(f"{len(xs)} clips of mode {a.mode!r} but {len(dicts)} label files: they are paired by position")
    nc = 12                                                     # search_best.py:100
    frames = [(int(x.shape[0]) - WIN_SIZE) // STEP_SIZE + WIN_SIZE // STEP_SIZE for x in xs]
    packed = utils.concat_labels([utils.pack_labels(d, T, nc) for d, T in zip(dicts, frames)])

    from . import evaluator
    nets = [evaluator.load_conv_temporal_model((a.batch, WIN_SIZE) + tuple(xs[0].shape[1:]), cfg, w) for cfg, w in saved]
    outs = evaluator.ensemble_models(nets, xs, win_size=WIN_SIZE, step_size=STEP_SIZE, batch_size=a.batch)
    dev = nets[0]._dev
    from .SELD_evaluation_metrics import STATE_NAMES, SELDMetrics_
    scorer = SELDMetrics_(doa_threshold=a.doa_threshold, nb_classes=nc, device=dev)
    sweep = lambda t: scorer.sweep_seld_scores(outs, packed, t, cand)
    thr, score, values, steps = search_thresholds(outs, packed, cand, a.start, a.doa_threshold, nc, sweep=sweep)
    state0, state = sweep(utils.thresh_table(a.start, nc))[1], sweep(thr)[1]
    result = {"mode": a.mode, "files": names, "candidates": [float(v) for v in cand], "start": float(a.start),
              "thresholds": [float(v) for v in thr],
              "start_score": state_score(state0), "start_metrics": [float(v) for v in seld_scores_from_state(state0)],
              "start_counters": dict(zip(STATE_NAMES, state0.tolist())),
              "score": score, "metrics": [float(v) for v in values], "counters": dict(zip(STATE_NAMES, state.tolist())),
              "steps": [{"class": c, "candidate": k, "threshold": float(cand[k]), "score": s} for c, k, s in steps]}
    with open(a.out, "w") as fid:
        json.dump(result, fid, indent=1)
    if a.write_answers:
        import torch
        os.makedirs(a.write_answers, exist_ok=True)
        t = torch.as_tensor(thr).to(dev)
        for name, (sed, doa) in zip(names, outs):
            utils.write_answer(a.write_answers, name + '.csv', sed > t, doa)
    print(f"start {result['start_score']:.5f} -> {score:.5f} in {len(steps)} steps; thresholds {[round(float(v), 2) for v in thr]}")
    return result


if __name__ == "__main__":
    main()
