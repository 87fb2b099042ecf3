"""CPU-side checks of the per-class threshold search: choose_step's rule, search_thresholds driven by the dict-based oracle
(tests/dcase_oracle.py through tests/dcase_sweep_cases.py), the case generator's seeds, seld_dcase_sweep's refusals and search_best.main's
configuration errors — none of them needs a device."""
import ctypes as C

import numpy as np
import pytest

import dcase_oracle as DO
import dcase_sweep_cases as SC


def _row(TP=0, FP=0, FN=0, S=0, D=0, I=0, Nref=10, total_DE=0.0, DE_TP=0, DE_FP=0, DE_FN=0):
    return np.array([TP, FP, FN, S, D, I, Nref, total_DE, DE_TP, DE_FP, DE_FN], np.float64)


def test_choose_step_rule():
    from seld_amd import search_best as SB
    good, mid, bad = _row(TP=8, FN=2, D=2, total_DE=80.0, DE_TP=8, DE_FN=2), _row(TP=6, FN=4, D=4, total_DE=60.0, DE_TP=6, DE_FN=4), \
        _row(TP=2, FN=8, D=8, total_DE=20.0, DE_TP=2, DE_FN=8)
    s_good, s_mid, s_bad = (DO.seld_score(DO.scores_from_state(r)) for r in (good, mid, bad))
    assert s_good < s_mid < s_bad
    assert SB.state_score(good) == s_good and SB.BASE_THRESHOLD == SC.BASE_THRESHOLD == (0.3, 0.35, 0.4, 0.45, 0.55, 0.6, 0.65, 0.7)
    # the first minimum in row-major (c, k) order wins a tie
    table = np.array([[bad, good, mid], [good, bad, good]])
    assert SB.choose_step(table, mid) == (0, 1, s_good)
    assert SB.choose_step(table[::-1], mid) == (0, 0, s_good)
    # a minimum equal to the base is no step, and neither is a higher one
    assert SB.choose_step(table, good) is None
    assert SB.choose_step(np.array([[bad, mid]]), good) is None
    assert SB.choose_step(np.array([[bad, mid]]), bad) == (0, 1, s_mid)
    # DE_TP = 0: LE = 180, not 0 / eps
    none = _row(FN=10, D=10, DE_FN=10)
    assert DO.scores_from_state(none)[2] == 180
    assert SB.state_score(none) == DO.seld_score(DO.scores_from_state(none)) == (10 / (10 + DO.EPS) + 1 + 180 / 180 + 1) / 4
    assert SB.choose_step(np.array([[none]]), bad) is None and SB.choose_step(np.array([[bad]]), none) == (0, 0, s_bad)


@pytest.mark.parametrize("kind,name", [("sweep", n) for n in SC.SWEEP_CASES] + [("search", n) for n in SC.SEARCH_CASES])
def test_every_named_seed_is_accepted_at_the_first_draw(kind, name):
    case = SC.sweep_case(name) if kind == "sweep" else SC.search_case(name)
    assert case[1] == 0, f"{kind} case {name}: {case[1]} redraws; name another seed"
    o = case[2]
    if kind == "sweep":
        nc, M = SC.SWEEP_CASES[name][0][2], len(SC.SWEEP_CASES[name][1])
        assert len(o.sweeps) == 1 and len(o.sweeps[0]) == nc * M + 1
        table, base = case[3], case[4]
        assert any(not np.array_equal(r, base) for r in table.reshape(-1, 11)), "no candidate changes a counter"
        assert base[DO.NAMES.index("DE_TP")] > 0


def test_sed_is_spread_across_the_candidate_range():
    files = SC.draw(3, 53, 6, 2, seed=0)
    sed = np.concatenate([f[0] for f in files])
    edges = np.array((0.0,) + SC.BASE_THRESHOLD + (1.0,))
    assert all(np.histogram(sed[:, c], edges)[0].min() > 0 for c in range(6)), "a class has no value between two neighbouring candidates"


def _literal_search(sweep, cand, nc, start, max_steps):
    """the loop of the issue, written out: sweep, first strict minimum in row-major order, set, repeat"""
    thr = np.full(nc, start, np.float32)
    steps = []
    while len(steps) < max_steps:
        table, base = sweep(thr)
        best, arg = DO.seld_score(DO.scores_from_state(base)), None
        for c in range(nc):
            for k in range(len(cand)):
                s = DO.seld_score(DO.scores_from_state(table[c, k]))
                if s < best:
                    best, arg = s, (c, k)
        if arg is None:
            break
        thr[arg[0]] = np.float32(cand[arg[1]])
        steps.append((arg[0], arg[1], best))
    return thr, steps


def test_search_thresholds_on_the_oracle():
    from seld_amd import search_best as SB
    shape, cand, start, _ = SC.SEARCH_CASES["two_files"]
    nc = shape[2]
    files, _, o, (thr, score, values, steps) = SC.search_case("two_files")
    assert thr.dtype == np.float32 and thr.shape == (nc,)
    want_thr, want_steps = _literal_search(SC.OracleSweep(files, nc, cand), cand, nc, start, nc * len(cand))
    assert steps == want_steps and np.array_equal(thr, want_thr)
    # it ends before the default bound, on a sweep that offers no better row
    assert 2 <= len(steps) < nc * len(cand) and len(o.sweeps) == len(steps) + 1
    assert SB.choose_step(*SC.OracleSweep(files, nc, cand)(thr)) is None
    # strictly falling, and below the flat 0.5 table
    flat = DO.score_files([f[:3] for f in files], 0.5, SC.DOA_THRESHOLD, nc)
    scores = [DO.seld_score(flat.scores())] + [s for _, _, s in steps]
    assert all(b < a for a, b in zip(scores[:-1], scores[1:])) and score == scores[-1] < scores[0]
    final = DO.score_files([f[:3] for f in files], thr, SC.DOA_THRESHOLD, nc)
    assert values == final.scores() and score == DO.seld_score(final.scores())
    # max_steps
    for m in (0, 1):
        o2 = SC.OracleSweep(files, nc, cand)
        t2, s2, _, st2 = SB.search_thresholds(None, None, cand, start, SC.DOA_THRESHOLD, nc, max_steps=m, sweep=o2)
        assert st2 == steps[:m] and s2 == scores[m] and len(o2.sweeps) == m + 1
        assert np.array_equal(t2, _literal_search(SC.OracleSweep(files, nc, cand), cand, nc, start, m)[0])
    with pytest.raises(ValueError):
        SB.search_thresholds(None, None, [], sweep=o)
    with pytest.raises(ValueError):
        SB.search_thresholds(None, None, [0.5] * 17, sweep=o)


def _sweep_args():
    """valid arguments of seld_dcase_sweep on host buffers the entry point must not reach with a bad argument beside them"""
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    off = (C.c_int32 * 3)(0, 10, 25)
    return [p, p, p, p, p, p, p, off, 2, 12, 3, 8, 10, 20.0, p, p, None]


def test_dcase_sweep_refuses_bad_arguments_without_a_device(seld_lib):
    from seld_amd import _lib
    bad = []
    for n_cand in (0, 17, -1):
        a = _sweep_args(); a[11] = n_cand; bad.append(a)
    for i in (3, 14):                                     # a NULL cand or table
        a = _sweep_args(); a[i] = None; bad.append(a)
    for i in (0, 1, 2, 4, 5, 6, 15):                      # the other pointers
        a = _sweep_args(); a[i] = None; bad.append(a)
    a = _sweep_args(); a[7] = C.cast(None, C.POINTER(C.c_int32)); bad.append(a)
    for off in ((0, 10, 10), (0, 10, 5), (1, 10, 25), (-3, 10, 25)):      # offsets that do not ascend from 0
        a = _sweep_args(); a[7] = (C.c_int32 * 3)(*off); bad.append(a)
    for idx, vals in ((8, (0, -1)), (9, (0, -4)), (10, (0, 9, -1)), (12, (0, 33, -2))):      # n_files, nc, K, block_size
        for v in vals:
            a = _sweep_args(); a[idx] = v; bad.append(a)
    a = _sweep_args(); a[7] = (C.c_int32 * 3)(0, 10, 2 ** 31 - 1); bad.append(a)             # N * nc past 32 bits
    for a in bad:
        assert _lib.ERR_NAMES[seld_lib.seld_dcase_sweep(*a)] == "SELD_ERR_INVALID", a[8:13]
    sb = seld_lib.seld_dcase_sweep_scratch_bytes
    # 4 segments at most: their table, then a counter word and eight averages per (segment, class, threshold): linear in each
    assert sb(25, 2, 12, 8, 10) == 4 * 2 * 4 + 4 * 12 * 9 * 9 * 8
    assert sb(25, 2, 12, 16, 10) == 4 * 2 * 4 + 4 * 12 * 17 * 9 * 8 and sb(25, 2, 1, 1, 10) == 4 * 2 * 4 + 4 * 2 * 9 * 8
    for args in ((25, 2, 12, 0, 10), (25, 2, 12, 17, 10), (25, 2, 0, 8, 10), (25, 2, 12, 8, 0), (25, 2, 12, 8, 33), (0, 1, 12, 8, 10),
                 (25, 0, 12, 8, 10), (2 ** 31, 1, 12, 8, 10)):
        assert sb(*args) == -1, args


def test_search_best_main_configuration_errors_without_a_device(tmp_path):
    from seld_amd import search_best as SB
    cfg, w = tmp_path / "SS5.json", tmp_path / "w.npz"
    cfg.write_text("{}")
    w.write_bytes(b"")
    common = ["--feat_path", str(tmp_path / "feat"), "--label_path", str(tmp_path / "lab"), "--ans_path", str(tmp_path)]
    with pytest.raises(ValueError, match="cfg.json:weights.npz"):
        SB.main(["--models", str(cfg)] + common)                                   # no weights beside the settings
    with pytest.raises(ValueError, match="no such file"):
        SB.main(["--models", f"{cfg}:{tmp_path / 'missing.npz'}"] + common)
    with pytest.raises(ValueError, match="--mode"):
        SB.main(["--models", f"{cfg}:{w}", "--mode", "train"] + common)
    with pytest.raises(ValueError, match="candidates"):
        SB.main(["--models", f"{cfg}:{w}", "--candidates"] + ["0.5"] * 17 + common)
    with pytest.raises(ValueError, match="feat_path"):
        SB.main(["--models", f"{cfg}:{w}"] + common)                               # the data set is looked for before any model is built
