"""seld_dcase_sweep, SELDMetrics_.sweep_seld_scores and seld_amd.search_best on the device.  The bar of a table row is the bits of the state
a fresh SELDMetrics_.update_seld_scores leaves for that row's threshold vector; the oracle (tests/dcase_oracle.py, cases from
tests/dcase_sweep_cases.py) is held to test_dcase_gpu.py's tolerances: equal integer counters, total_DE within DE_TOL per averaged track."""
import ctypes as C
import functools
import json

import numpy as np
import pytest
import torch

import dcase_oracle as DO
import dcase_sweep_cases as SC
from test_dcase_gpu import DE_TOL, INT_NAMES

pytestmark = pytest.mark.gpu

DE = DO.NAMES.index("total_DE")
# (files, T, nc, K, M): name of the margin-checked case, or (seed, candidates, base) of a case that is compared with the scorer only
BIT_CASES = {
    (2, 23, 3, 2, 3): "two_files",                   # two files, ragged tail segments
    (1, 7, 1, 4, 1): "one_segment",                  # one segment, one class, one candidate
    (3, 53, 12, 3, 8): "twelve_classes",             # BASE_THRESHOLD on a linspace(0.2, 0.8, 12) base table
    (1, 10, 12, 1, 16): (0, tuple(np.linspace(0.2, 0.95, 16).astype(np.float32).tolist()), 0.5),      # the candidate maximum
    (1, 2570, 2, 1, 2): (0, (0.4, 0.6), 0.5),        # 257 segments: past the 64-thread blocks and the reduction's 256-row stride
}


@functools.lru_cache(maxsize=None)
def _case(shape):
    """-> (files, candidates, base table) of a BIT_CASES shape"""
    what = BIT_CASES[shape]
    if isinstance(what, str):
        assert SC.SWEEP_CASES[what][0] == shape[:4] and len(SC.SWEEP_CASES[what][1]) == shape[4]
        return SC.sweep_case(what)[0], SC.SWEEP_CASES[what][1], SC.SWEEP_CASES[what][2]
    seed, cand, base = what
    assert len(cand) == shape[4]
    return SC.draw(*shape[:4], seed=seed), cand, base


class _Device:
    """the files of a case on the device, their labels packed once, and one scorer that is reset between rows"""

    def __init__(self, files, nc):
        from seld_amd import utils
        from seld_amd.SELD_evaluation_metrics import SELDMetrics_
        self.nc = nc
        self.pred = [(torch.as_tensor(f[0]).cuda(), torch.as_tensor(f[1]).cuda()) for f in files]
        self.gt = utils.concat_labels([utils.pack_labels(f[2], f[0].shape[0], nc) for f in files])
        self.m = SELDMetrics_(doa_threshold=SC.DOA_THRESHOLD, nb_classes=nc)

    def sweep(self, base, cand):
        return self.m.sweep_seld_scores(self.pred, self.gt, base, cand)

    def update(self, thr):
        """the state of a fresh update_seld_scores at `thr`"""
        self.m.reset_states()
        self.m.update_seld_scores(self.pred, self.gt, sed_thresh=[float(v) for v in thr])
        out = self.m.state.cpu().numpy().copy()
        self.m.reset_states()
        return out

    def raw_sweep(self, base, cand, table):
        """seld_dcase_sweep itself, into a table the caller made"""
        from seld_amd import _lib, utils
        m, gt = self.m, self.gt
        sed = torch.cat([s for s, _ in self.pred]).contiguous()
        doa = torch.cat([d for _, d in self.pred]).contiguous()
        xyz, slot, n = gt.to_device(sed.device)
        thr = torch.as_tensor(utils.thresh_table(base, self.nc)).cuda()
        cd = torch.as_tensor(np.asarray(cand, np.float32)).cuda()
        n_files = len(self.pred)
        need = int(m.lib.seld_dcase_sweep_scratch_bytes(gt.n_frames, n_files, self.nc, len(cand), utils.SEGMENT_FRAMES))
        assert need > 0
        scratch = torch.empty((need + 7) // 8, dtype=torch.int64, device=sed.device)
        _lib.check(m.lib.seld_dcase_sweep(sed.data_ptr(), doa.data_ptr(), thr.data_ptr(), cd.data_ptr(), xyz.data_ptr(), slot.data_ptr(),
                                          n.data_ptr(), gt.file_off.ctypes.data_as(C.POINTER(C.c_int32)), n_files, self.nc, gt.K, len(cand),
                                          utils.SEGMENT_FRAMES, float(SC.DOA_THRESHOLD), table.data_ptr(), scratch.data_ptr(),
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        return table


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _rows(table, base):
    return list(table.reshape(-1, 11)) + [base]


def _against_scorer(dev, base, cand):
    table, b = dev.sweep(base, cand)
    assert table.shape == (dev.nc, len(cand), 11) and b.shape == (11,) and table.dtype == b.dtype == np.float64
    thrs = SC.row_thresholds(base, cand, dev.nc)
    for i, (row, thr) in enumerate(zip(_rows(table, b), thrs)):
        want = dev.update(thr)
        assert np.array_equal(_bits(row), _bits(want)), (i, thr.tolist(), row.tolist(), want.tolist())
    return table, b


def _against_oracle(rows, scorers):
    for i, (row, sc) in enumerate(zip(rows, scorers)):
        got, want = dict(zip(DO.NAMES, row)), dict(zip(DO.NAMES, sc.state()))
        for n in INT_NAMES:
            assert got[n] == want[n], (i, n, got[n], want[n])
        assert abs(got["total_DE"] - want["total_DE"]) <= DE_TOL * max(want["DE_TP"], 1), (i, got["total_DE"], want["total_DE"])


@pytest.mark.parametrize("shape", list(BIT_CASES))
def test_every_row_has_the_bits_of_a_fresh_update(shape):
    files, cand, base = _case(shape)
    table, b = _against_scorer(_Device(files, shape[2]), base, cand)
    assert b[DO.NAMES.index("Nref")] > 0 and len({r.tobytes() for r in _rows(table, b)}) > 1


@pytest.mark.parametrize("shape", [s for s, w in BIT_CASES.items() if isinstance(w, str)])
def test_every_row_against_the_oracle(shape):
    files, cand, base = _case(shape)
    o = SC.sweep_case(BIT_CASES[shape])[2]
    table, b = _Device(files, shape[2]).sweep(base, cand)
    _against_oracle(_rows(table, b), [sc for _, sc in o.sweeps[0]])


def _oracle_rows(files, nc, base, cand):
    o = SC.OracleSweep(files, nc, cand)
    o(np.broadcast_to(np.asarray(base, np.float32), (nc,)).copy())
    assert SC.objection(o.sweeps, choice=False) is None
    return [sc for _, sc in o.sweeps[0]]


def test_a_value_equal_to_a_candidate_is_inactive():
    files, _, _ = _case((2, 23, 3, 2, 3))
    cand, c = (0.35, 0.5, 0.65), 1
    at = np.float32(0.35)
    # segment 1 of file 0, class c: one frame decides whether the class is predicted there.  A frame with a reference entry if there is one
    # (FN becomes TP or FP), else any frame (an FP appears)
    with_ref = [t for t in range(10, 20) if any(r[0] == c for r in files[0][2].get(t, []))]
    frame = with_ref[0] if with_ref else 13

    def with_value(v):
        sed = files[0][0].copy()
        sed[10:20, c] = 0.01
        sed[frame, c] = v
        return [(sed,) + files[0][1:]] + list(files[1:])
    equal, off, above = (_Device(with_value(v), 3).sweep(0.5, cand)[0] for v in (at, np.float32(0.01), np.nextafter(at, np.float32(1))))
    assert np.array_equal(_bits(equal[c, 0]), _bits(off[c, 0]))
    assert not np.array_equal(above[c, 0, [0, 1, 2]], equal[c, 0, [0, 1, 2]])          # one ulp above it, TP, FP or FN moves
    assert np.array_equal(_bits(equal[c, 1:]), _bits(above[c, 1:]))                    # and 0.5 and 0.65 see neither
    table, b = _Device(with_value(at), 3).sweep(0.5, cand)
    _against_oracle(_rows(table, b), _oracle_rows(with_value(at), 3, 0.5, cand))


def test_candidate_order_duplicates_and_extremes():
    files, _, _ = _case((2, 23, 3, 2, 3))
    dev = _Device(files, 3)
    sed = np.concatenate([f[0] for f in files])
    table, b = _against_scorer(dev, 0.5, (0.6, 0.3, 0.6))              # descending, then a duplicate
    assert np.array_equal(_bits(table[:, 0]), _bits(table[:, 2])) and not np.array_equal(table[:, 0], table[:, 1])
    # a candidate above every value: with the other classes off as well, the class leaves no TP and no FP; below every value: all frames on
    hi, lo = float(sed.max()) + 0.5, float(sed.min()) / 2
    assert lo > 0
    table, b = _against_scorer(dev, hi, (hi, 0.5, lo))
    tp, fp, de_tp = (DO.NAMES.index(n) for n in ("TP", "FP", "DE_TP"))
    assert b[tp] == b[fp] == b[de_tp] == 0 and b[DO.NAMES.index("FN")] > 0
    assert np.array_equal(_bits(table[:, 0]), _bits(np.broadcast_to(b, (3, 11))))
    assert all(table[c, 1, tp] + table[c, 1, fp] > 0 for c in range(3))
    for base, cand in ((0.5, (hi, lo)), (hi, (hi, 0.5, lo))):
        table, b = dev.sweep(base, cand)
        _against_oracle(_rows(table, b), _oracle_rows(files, 3, base, cand))


def test_the_table_is_overwritten_and_repeatable_and_the_state_is_left_alone():
    files, cand, base = _case((2, 23, 3, 2, 3))
    dev = _Device(files, 3)
    dev.m.update_seld_scores(dev.pred, dev.gt, sed_thresh=0.4)
    before = dev.m.state.cpu().numpy().copy()
    assert before.sum() > 0
    table, b = dev.sweep(base, cand)
    assert np.array_equal(_bits(dev.m.state.cpu().numpy()), _bits(before))
    raw = []
    for fill in (float("nan"), 1e300):
        t = torch.full((3 * len(cand) + 1, 11), fill, dtype=torch.float64, device="cuda")
        raw.append(dev.raw_sweep(base, cand, t).cpu().numpy())
        assert np.isfinite(raw[-1]).all()
    assert np.array_equal(_bits(raw[0]), _bits(raw[1]))
    assert np.array_equal(_bits(raw[0][:-1].reshape(3, len(cand), 11)), _bits(table)) and np.array_equal(_bits(raw[0][-1]), _bits(b))
    with pytest.raises(ValueError):
        dev.sweep(base, [0.5] * 17)
    with pytest.raises(ValueError):
        dev.m.sweep_seld_scores(dev.pred[:1], dev.gt, base, cand)


def test_search_on_the_device_takes_the_oracle_steps():
    from seld_amd import search_best as SB
    shape, cand, start, _ = SC.SEARCH_CASES["six_classes"]
    files, _, _, (thr_o, score_o, _, steps_o) = SC.search_case("six_classes")
    dev = _Device(files, shape[2])
    thr, score, values, steps = SB.search_thresholds(dev.pred, dev.gt, cand, start, SC.DOA_THRESHOLD, shape[2])
    print(steps, steps_o)
    assert [(c, k) for c, k, _ in steps] == [(c, k) for c, k, _ in steps_o] and len(steps) >= 2
    assert np.array_equal(thr, thr_o) and abs(score - score_o) <= DE_TOL / 180 / 4
    state = dev.update(thr)
    assert score == SB.state_score(state) and tuple(values) == tuple(SB.seld_scores_from_state(state))
    assert steps[-1][2] == score and score < SB.state_score(dev.update(np.full(shape[2], start, np.float32)))
    # packing inside the call gives the same walk
    from seld_amd import utils
    again = SB.search_thresholds(dev.pred, [utils.pack_labels(f[2], f[0].shape[0], shape[2]) for f in files], cand, start, nb_classes=shape[2],
                                 max_steps=2)
    assert again[3] == steps[:2]


def test_search_best_main_on_a_tiny_dataset(tmp_path):
    """one fold-5 clip of 800 frames (160 label frames), the small SS5 configuration with the weights a fresh model saves"""
    from conv_temporal_oracle import SS5_SMALL
    from seld_amd import models, search_best as SB, utils
    feat, lab, meta = tmp_path / "feat", tmp_path / "lab", tmp_path / "metadata_dev" / "dev-val"
    for d in (feat, lab, meta):
        d.mkdir(parents=True)
    rng = np.random.default_rng(0)
    T = 160
    gt = {}
    for name, frames in (("fold5_room1_mix000", 800), ("fold6_room1_mix000", 300)):          # the fold-6 clip is not part of `val`
        np.save(feat / (name + ".npy"), rng.standard_normal((frames, 64, 7)).astype(np.float32))
        np.save(lab / (name + ".npy"), np.zeros((frames // 5, 48), np.float32))
    on = rng.random((T, 12)) < 0.3
    for t, c in zip(*np.nonzero(on)):
        gt.setdefault(int(t), []).append([int(c), int(rng.integers(-180, 180)), int(rng.integers(-45, 46)), 0])
    DO.write_metadata_csv(meta / "fold5_room1_mix000.csv", gt)
    cfg, weights = tmp_path / "SS5.json", tmp_path / "w.npz"
    cfg.write_text(json.dumps(SS5_SMALL))
    models.conv_temporal((1, 300, 64, 7), dict(SS5_SMALL)).save_weights(str(weights))
    out, ans = tmp_path / "thresholds.json", tmp_path / "answers"
    res = SB.main(["--models", f"{cfg}:{weights}", "--feat_path", str(feat), "--label_path", str(lab), "--ans_path",
                   str(tmp_path / "metadata_dev"), "--mode", "val", "--out", str(out), "--write_answers", str(ans), "--batch", "32"])
    saved = json.loads(out.read_text())
    assert saved == json.loads(json.dumps(res)) and saved["files"] == ["fold5_room1_mix000"]
    allowed = {float(np.float32(v)) for v in SB.BASE_THRESHOLD + (0.5,)}
    assert len(saved["thresholds"]) == 12 and all(v in allowed for v in saved["thresholds"])
    assert saved["score"] <= saved["start_score"] and len(saved["metrics"]) == len(saved["start_metrics"]) == 4
    assert [s["score"] for s in saved["steps"]] == sorted((s["score"] for s in saved["steps"]), reverse=True)
    assert saved["score"] == SB.state_score([saved["counters"][n] for n in DO.NAMES])
    # the answer files, read back and scored by the dict path, give the reported counters
    pred = utils.load_output_format_file(str(ans / "fold5_room1_mix000.csv"))
    assert pred == DO.load_csv(ans / "fold5_room1_mix000.csv")
    sc = DO.Scorer(SC.DOA_THRESHOLD, 12)
    sc.update(DO.segment_labels(pred, T), DO.segment_labels(DO.polar_to_cartesian(gt), T))
    print(saved["counters"], sc.c, saved["steps"])
    _against_oracle([np.array([saved["counters"][n] for n in DO.NAMES])], [sc])
