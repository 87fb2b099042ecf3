"""Time-domain mixing without a GPU: the oracle (tests/tdm_oracle.py) on a hand-computed case, that the plans of tests/tdm_cases.py meet the
situations tests/test_tdm_gpu.py names, the host side of data_loader (frame counts, draws, plan checks, csv / wav / bank readers), the flags,
and every refusal of seld_aug_tdm_labels / seld_aug_tdm_mix (both validate before their first HIP call: dummy pointers are never
dereferenced and no device is needed)."""
import json
import wave

import numpy as np
import pytest
import torch

import tdm_cases as TC
import tdm_oracle as TO

OK, INVALID, UNSUPPORTED = 0, -1, -2
P = 0x1000          # a non-null, 16-byte aligned pointer that is never dereferenced


# ---------------------------------------------------------------- the oracle
def test_oracle_on_a_hand_computed_case():
    """T = 6, nc = 2, K = 2, max_per_frame = 1, one channel, 2 samples per label frame.  Class 0 is active in frame 1.
    k0 = (cls 0, st 3, offset 1, td 0): frame 1 is taken (0), frames 2 and 3 are free -> v = [0, 1, 1]; they now hold class 0.
    k1 = (cls 1, st 3, offset 3, td 1): frame 3 is full only because k0 added there -> v = [0, 1, 1]."""
    y = np.zeros((1, 6, 8), np.float32)
    y[0, 1] = [1, 0, 0.5, 0, 0.5, 0, 0.25, 0]                      # [act0 act1 | x0 x1 | y0 y1 | z0 z1]
    b0 = np.array([[1, 0, 0.1 * (r + 1), 0, 0.2, 0, 0.3, 0] for r in range(4)], np.float32)
    b1 = np.array([[0, 1, 0, -0.1 * (r + 1), 0, 0.5, 0, 0.6] for r in range(5)], np.float32)
    x = np.arange(12, dtype=np.float32).reshape(1, 1, 12)
    w0 = 100 + np.arange(8, dtype=np.float32).reshape(1, 8)        # class 0: frames of samples (100, 101), (102, 103), ...
    w1 = 200 + np.arange(10, dtype=np.float32).reshape(1, 10)
    plan = np.array([[[0, 3, 1, 0], [1, 3, 3, 1]]])
    xo, yo, valid = TO.tdm_aug(x, y, [w0, w1], [b0, b1], plan, spf=2, max_per_frame=1)
    np.testing.assert_array_equal(valid, np.array([[[0, 1, 1], [0, 1, 1]]], np.float32))
    want_y = y.copy()
    want_y[0, 2] = b0[1]
    want_y[0, 3] = b0[2]
    want_y[0, 4] = b1[2]
    want_y[0, 5] = b1[3]
    np.testing.assert_array_equal(yo, want_y)
    want_x = x.copy()
    want_x[0, 0, 4:8] += [102, 103, 104, 105]                      # k0: clip frames 2, 3 <- class-0 frames 1, 2
    want_x[0, 0, 8:12] += [204, 205, 206, 207]                     # k1: clip frames 4, 5 <- class-1 frames 2, 3
    np.testing.assert_array_equal(xo, want_x)
    np.testing.assert_array_equal(x[0, 0], np.arange(12))          # the inputs are not modified


def test_oracle_skips_an_insertion_without_a_valid_frame():
    y = np.zeros((1, 4, 4), np.float32)
    y[0, :, 0] = 1
    x = np.ones((1, 2, 8), np.float32)
    xo, yo, valid = TO.tdm_aug(x, y, [np.full((2, 8), 7, np.float32)], [np.ones((4, 4), np.float32)], np.array([[[0, 4, 0, 0]]]), spf=2)
    np.testing.assert_array_equal(valid, np.zeros((1, 1, 4), np.float32))
    np.testing.assert_array_equal(xo, x)
    np.testing.assert_array_equal(yo, y)


def test_gpu_cases_meet_their_situations():
    """the validity vectors written by hand in tdm_cases.labels_case's docstring are what the oracle computes, and the edge conditions hold"""
    y, plan, expect = TC.labels_case()
    tdm_x, tdm_y = TC.make_bank(TC.BANK_ROWS, TC.NC, 4, 8, seed=1)
    _, yo, valid = TO.tdm_aug(TC.waves(3, 4, TC.T * 8, 2), y, tdm_x, tdm_y, plan, 8, TC.MAX_PER_FRAME)
    for (b, k), v in expect.items():
        st = plan[b, k, 1]
        assert len(v) == st
        np.testing.assert_array_equal(valid[b, k, :st], np.array(v, np.float32), err_msg=f"clip {b} insertion {k}")
        assert (valid[b, k, st:] == 0).all()
    assert len(expect) == 12
    cls, st, off, td = (plan[..., i] for i in range(4))
    rows = np.array(TC.BANK_ROWS)
    assert (off == 0).any() and (off + st == TC.T).any() and (st == 1).any() and (td + st == rows[cls]).any()
    assert (valid[0, 3] == 0).all()                                             # an insertion with no valid frame
    assert ((valid > 0) & (valid < 1)).any()                                    # fractional
    assert (np.diff(cls[1, :3]) == 0).all()                                     # the same class again
    assert not np.array_equal(yo, y)
    # T = 320: an insertion longer than a workgroup, partly valid
    y2, plan2, rows2 = TC.long_case()
    bx, by = TC.make_bank(rows2, TC.NC, 1, 4, seed=3)
    _, _, v2 = TO.tdm_aug(TC.waves(2, 1, 320 * 4, 4), y2, bx, by, plan2, 4, TC.MAX_PER_FRAME)
    assert plan2[..., 1].max() == 300 and 0 < v2[0, 0].sum() < 300 and v2[0, 0, 256:].sum() > 0
    assert v2[1, 1, 20:].sum() == 0 and v2[1, 1, :20].sum() > 0                 # the second pass of the same class fits only where the first did not reach


# ---------------------------------------------------------------- data_loader, host side
def test_frame_count_quirk():
    """int(sec / label_resolution) as Python evaluates it (data_loader.py:196-197): 0.3 / 0.1 = 2.9999999999999996 -> 2"""
    from seld_amd import data_loader as dl
    assert [dl.tdm_frames(s) for s in (0.5, 0.3, 1, 3)] == [5, 2, 10, 30]


def test_draw_tdm_ranges_and_frequencies():
    from seld_amd import data_loader as dl
    rows = [12, 25, 40]
    plan = dl.draw_tdm(np.random.default_rng(0), 2000, 60, rows, 3, 5, 10)
    assert plan.shape == (2000, 3, 4) and plan.dtype == np.int32
    cls, st, off, td = (plan[..., i] for i in range(4))
    assert cls.min() == 0 and cls.max() == 2
    assert st.min() == 5 and st.max() == 9                                      # [min_frames, max_frames)
    assert off.min() >= 0 and (off < 60 - st).all() and (off == 60 - st - 1).any()        # [0, T - st)
    assert td.min() >= 0 and (td < np.array(rows)[cls] - st).all() and (td == np.array(rows)[cls] - st - 1).any()
    # class frequencies follow 1 / bank_rows: 6 000 draws, 4.5 sigma of the binomial
    p = 1 / np.array(rows, float)
    p /= p.sum()
    freq = np.bincount(cls.ravel(), minlength=3) / cls.size
    assert (np.abs(freq - p) < 4.5 * np.sqrt(p * (1 - p) / cls.size)).all(), (freq, p)
    a = dl.draw_tdm(np.random.default_rng(7), 5, 60, rows, 2, 5, 10)
    np.testing.assert_array_equal(a, dl.draw_tdm(np.random.default_rng(7), 5, 60, rows, 2, 5, 10))
    assert dl.draw_tdm(np.random.default_rng(0), 4, 60, rows, 0, 5, 10).shape == (4, 0, 4)
    for bad in (dict(T=60, rows=rows, lo=5, hi=5),          # st: maxval <= minval
                dict(T=9, rows=rows, lo=5, hi=10),          # offset: T - st <= 0 for st = 9
                dict(T=60, rows=[9, 40], lo=5, hi=10),      # td_offset: bank_rows - st <= 0
                dict(T=60, rows=[], lo=5, hi=10)):
        with pytest.raises(ValueError):
            dl.draw_tdm(np.random.default_rng(0), 4, bad["T"], bad["rows"], 2, bad["lo"], bad["hi"])
    with pytest.raises(ValueError):
        dl.draw_tdm(np.random.default_rng(0), 4, 60, rows, 33, 5, 10)


def _host_args():
    tdm_x, tdm_y = TC.make_bank((12, 25), 2, 4, 8, seed=0)
    return torch.zeros(2, 4, 40 * 8), torch.zeros(2, 40, 8), tdm_x, tdm_y


def test_tdm_aug_refuses_host_tensors():
    from seld_amd import data_loader as dl
    x, y, tdm_x, tdm_y = _host_args()
    good = np.array([[[0, 5, 0, 0]], [[1, 5, 35, 20]]], np.int32)
    with pytest.raises(ValueError, match="CUDA"):
        dl.TDM_aug(x, y, tdm_x, tdm_y, sr=80, draws=good)
    with pytest.raises(ValueError, match="CUDA"):
        dl.TDM_aug(x.numpy(), y.numpy(), tdm_x, tdm_y, sr=80, draws=good)
    with pytest.raises(ValueError, match="CUDA"):
        dl.TDM_aug([x[0], x[1]], y, tdm_x, tdm_y, sr=80, min_overlap_sec=0.5, max_overlap_sec=1, rng=np.random.default_rng(0))


@pytest.mark.parametrize("draws, what", [
    (np.zeros((2, 1, 4), np.float32), "integers"),
    (np.zeros((2, 4), np.int32), "must be"),
    (np.zeros((3, 1, 4), np.int32), "must be"),
    (np.zeros((2, 1, 3), np.int32), "must be"),
    (np.zeros((2, 33, 4), np.int32), "at most"),
    (np.array([[[2, 5, 0, 0]], [[0, 5, 0, 0]]], np.int32), "class"),
    (np.array([[[-1, 5, 0, 0]], [[0, 5, 0, 0]]], np.int32), "class"),
    (np.array([[[0, 5, 36, 0]], [[0, 5, 0, 0]]], np.int32), "outside the clip"),
    (np.array([[[0, 5, -1, 0]], [[0, 5, 0, 0]]], np.int32), "outside the clip"),
    (np.array([[[0, -1, 3, 0]], [[0, 5, 0, 0]]], np.int32), "outside the clip"),
    (np.array([[[0, 5, 0, 8]], [[0, 5, 0, 0]]], np.int32), "bank track"),
    (np.array([[[0, 5, 0, -1]], [[0, 5, 0, 0]]], np.int32), "bank track"),
])
def test_tdm_aug_refuses_bad_draws(draws, what):
    """range, dtype and shape of `draws` are judged on the host, before any tensor is looked at"""
    from seld_amd import data_loader as dl
    x, y, tdm_x, tdm_y = _host_args()
    with pytest.raises(ValueError, match=what):
        dl.TDM_aug(x, y, tdm_x, tdm_y, sr=80, draws=draws)
    with pytest.raises(ValueError, match=what):
        dl.check_tdm_draws(draws, 2, 40, [12, 25])


def test_check_tdm_draws_accepts_the_edges():
    from seld_amd import data_loader as dl
    d = dl.check_tdm_draws([[[1, 25, 15, 0], [0, 0, 40, 12]]], 1, 40, [12, 25])      # offset + st = T, td + st = rows, an empty insertion
    assert d.dtype == np.int32 and d.flags.c_contiguous and d.shape == (1, 2, 4)


def test_extract_labels_on_a_five_line_csv(tmp_path):
    from seld_amd import data_loader as dl, feature_extractor as fe
    assert dl.extract_labels is fe.extract_labels
    p = tmp_path / "fold1_room1_mix001.csv"
    p.write_text("0,1,0,0,0\n0,3,1,90,0\n2,1,0,180,30\n4,0,0,-90,-45\n4,2,0,45,90\n")
    got = fe.extract_labels(str(p), n_classes=4)
    want = np.zeros((5, 4, 4), np.float32)                 # [frame, (act, x, y, z), class]
    r = np.sqrt(0.5)
    want[0, :, 1] = [1, 1, 0, 0]
    want[0, :, 3] = [1, 0, 1, 0]
    want[2, :, 1] = [1, -np.sqrt(0.75), 0, 0.5]
    want[4, :, 0] = [1, 0, -r, -r]
    want[4, :, 2] = [1, 0, 0, 1]
    assert got.shape == (5, 16) and got.dtype == np.float32
    np.testing.assert_allclose(got, want.reshape(5, 16), atol=1e-7)
    assert fe.extract_labels(str(p), n_classes=4, max_frames=9).shape == (9, 16)
    assert fe.extract_labels(str(p), n_classes=4, max_frames=3).shape == (5, 16)
    assert fe.extract_labels(str(p)).shape == (5, 56)


def _write_wav(path, pcm, width=2):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(pcm.shape[1])
        w.setsampwidth(width)
        w.setframerate(24000)
        w.writeframes(pcm.astype("<i2" if width == 2 else "<i4").tobytes())


def test_load_wav_and_label(tmp_path):
    from seld_amd import data_loader as dl
    wavs, labs = tmp_path / "foa_dev", tmp_path / "metadata_dev"
    wavs.mkdir(), labs.mkdir()
    rng = np.random.default_rng(0)
    pcm = {}
    for fold in (1, 3, 5, 6):
        name = f"fold{fold}_room1_mix000"
        pcm[fold] = rng.integers(-32768, 32768, (100 + fold, 4)).astype(np.int16)
        pcm[fold][0] = [-32768, 32767, 0, 1]
        _write_wav(wavs / (name + ".wav"), pcm[fold])
        (labs / (name + ".csv")).write_text(f"0,1,0,0,0\n{3 + fold},2,0,90,0\n")
    x, y = dl.load_wav_and_label(str(wavs), str(labs), "train", n_classes=3, max_label_length=6)
    assert len(x) == 2 and len(y) == 2                                         # folds 1 and 3 of 1-4
    for got, fold in zip(x, (1, 3)):
        assert got.dtype == np.float32 and got.shape == (4, 100 + fold)
        np.testing.assert_array_equal(got, pcm[fold].T.astype(np.float32) / np.float32(32768))
    assert x[0][0, 0] == -1.0 and x[0][1, 0] == np.float32(32767 / 32768)
    assert [l.shape for l in y] == [(6, 12), (6, 12)]
    assert y[0][4, 2] == 1 and y[0][5].sum() == 0                              # 5 frames padded to 6
    assert y[1][5].sum() == 0 and y[1][0, 1] == 1                              # 7 frames trimmed to 6: the event of frame 6 is gone
    xv, yv = dl.load_wav_and_label(str(wavs), str(labs), "val", n_classes=3)
    assert len(xv) == 1 and xv[0].shape == (4, 105) and yv[0].shape == (600, 12)
    assert len(dl.load_wav_and_label(str(wavs), str(labs), "test", n_classes=3)[0]) == 1
    (labs / "fold2_room1_mix000.csv").write_text("0,1,0,0,0\n")               # a label without its wav
    with pytest.raises(ValueError, match="not matched"):
        dl.load_wav_and_label(str(wavs), str(labs), "train", n_classes=3)
    (labs / "fold2_room1_mix000.csv").unlink()
    _write_wav(wavs / "fold2_room1_mix000.wav", rng.integers(-100, 100, (50, 4)), width=4)
    (labs / "fold2_room1_mix000.csv").write_text("0,1,0,0,0\n")
    with pytest.raises(ValueError, match="16-bit"):
        dl.load_wav_and_label(str(wavs), str(labs), "train", n_classes=3)


def test_get_tdmset(tmp_path):
    from seld_amd import data_loader as dl
    d = tmp_path / "foa_dev_tdm"
    d.mkdir()
    tdm_x, tdm_y = TC.make_bank((3, 5), 2, 4, 2400, seed=0, extra=7)
    for k in range(2):
        np.save(d / f"tdm_noise_{k}.npy", tdm_x[k].astype(np.float64))
        np.save(d / f"tdm_label_{k}.npy", tdm_y[k])
    gx, gy = dl.get_TDMset(str(tmp_path))
    assert len(gx) == 2 and all(a.dtype == np.float32 for a in gx + gy)
    for k in range(2):
        np.testing.assert_array_equal(gx[k], tdm_x[k])
        np.testing.assert_array_equal(gy[k], tdm_y[k])
    np.save(d / "tdm_noise_1.npy", tdm_x[1][:, :5 * 2400 - 1])                 # one sample short of its 5 label frames
    with pytest.raises(ValueError, match="fewer"):
        dl.get_TDMset(str(tmp_path))


def test_use_tdm_flags(tmp_path, seldnet_config):
    from seld_amd import params
    d = tmp_path / "model_config"
    d.mkdir()
    (d / "seldnet.json").write_text(json.dumps(seldnet_config))
    paths = {"--tdm_wav_path": "w", "--tdm_label_path": "l", "--tdm_bank_path": "b"}
    flat = lambda keys: [a for k in keys for a in (k, paths[k])]
    config, _ = params.get_param(["--name", "x", "--use_tdm"] + flat(paths), model_config_dir=str(d))
    assert config.use_tdm and (config.tdm_wav_path, config.tdm_label_path, config.tdm_bank_path) == ("w", "l", "b") and config.tdm_epoch == 2
    for missing in paths:
        with pytest.raises(ValueError, match=missing) as e:
            params.get_param(["--name", "x", "--use_tdm"] + flat(k for k in paths if k != missing), model_config_dir=str(d))
        assert not any(k in str(e.value) for k in paths if k != missing)
    with pytest.raises(ValueError, match="--tdm_wav_path, --tdm_label_path, --tdm_bank_path"):
        params.get_param(["--name", "x", "--use_tdm"], model_config_dir=str(d))
    assert not params.get_param(["--name", "x"] + flat(paths), model_config_dir=str(d))[0].use_tdm      # the paths alone switch nothing on


# ---------------------------------------------------------------- the entry points' refusals
def _labels(lib, **kw):
    a = dict(y=P, B=2, T=40, W=12, bank_y=P, bank_row0=P, bank_rows=P, n_cls=3, plan=P, K=4, max_per_frame=2, valid=P, ld_valid=10, stream=None)
    a.update(kw)
    return lib.seld_aug_tdm_labels(*a.values())


def _mix(lib, **kw):
    a = dict(x_in=P, x_out=P, B=2, C=4, N=320, T=40, spf=8, bank_x=P, bank_s0=P, n_cls=3, plan=P, K=4, valid=P, ld_valid=10, stream=None)
    a.update(kw)
    return lib.seld_aug_tdm_mix(*a.values())


@pytest.mark.parametrize("kw, want", [
    (dict(y=None), INVALID), (dict(bank_y=None), INVALID), (dict(bank_row0=None), INVALID), (dict(bank_rows=None), INVALID),
    (dict(plan=None), INVALID), (dict(valid=None), INVALID), (dict(plan=P + 4), INVALID),
    (dict(B=0), INVALID), (dict(T=0), INVALID), (dict(W=0), INVALID), (dict(n_cls=0), INVALID), (dict(B=-1), INVALID),
    (dict(W=10), INVALID), (dict(K=-1), INVALID), (dict(ld_valid=0), INVALID), (dict(n_cls=4), INVALID),
    (dict(K=33), UNSUPPORTED), (dict(B=1 << 24), UNSUPPORTED),
    (dict(K=0), OK), (dict(K=0, plan=None, valid=None), OK),
    (dict(K=0, y=None), INVALID), (dict(K=0, W=10), INVALID),
])
def test_labels_entry_point_refusals(seld_lib, kw, want):
    assert _labels(seld_lib, **kw) == want


@pytest.mark.parametrize("kw, want", [
    (dict(x_in=None), INVALID), (dict(x_out=None), INVALID), (dict(bank_x=None), INVALID), (dict(bank_s0=None), INVALID),
    (dict(plan=None), INVALID), (dict(valid=None), INVALID), (dict(plan=P + 8), INVALID),
    (dict(B=0), INVALID), (dict(C=0), INVALID), (dict(T=0), INVALID), (dict(spf=0), INVALID), (dict(n_cls=0), INVALID),
    (dict(K=-1), INVALID), (dict(ld_valid=0), INVALID), (dict(N=319), INVALID),
    (dict(K=33), UNSUPPORTED), (dict(B=1 << 20, T=16, N=128), UNSUPPORTED),
    (dict(K=0), OK), (dict(K=0, plan=None, valid=None), OK),             # in place: nothing to do, nothing enqueued
    (dict(K=0, N=319), INVALID), (dict(K=0, bank_x=None), INVALID),
])
def test_mix_entry_point_refusals(seld_lib, kw, want):
    assert _mix(seld_lib, **kw) == want
