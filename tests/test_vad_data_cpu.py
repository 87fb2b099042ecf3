"""The voice-activity data path without a device: the host entries of csrc/vad_feat.hip (mel matrix, frame counts) against the fp64
restatement tests/vad_data_oracle.py, pins of that restatement, every refusal of the C entries and of the Python loaders, and the room plain
fp32 leaves under the GPU tests' bar (helpers.check: 1e-4 of the tensor's maximum) on the very cases tests/test_vad_data_gpu.py runs."""
import ctypes as C
import os
import wave

import numpy as np
import pytest
import torch

import vad_data_oracle as D
from conftest import ROOT
from helpers import REL_TOL, rel_err

NEW_SYMBOLS = ("seld_vad_feat_create", "seld_vad_feat_destroy", "seld_vad_feat_frames", "seld_vad_mel_matrix_host", "seld_vad_feat_extract",
               "seld_vad_frame_labels", "seld_vad_gather", "seld_vad_score_update")
INVALID, UNSUPPORTED = -1, -2


def lib_mel(lib, n_mels, n_bins, sr, lo=0.0, hi=None):
    w = np.full((n_bins, n_mels), np.nan, np.float32)
    rc = lib.seld_vad_mel_matrix_host(n_mels, n_bins, sr, lo, sr // 2 if hi is None else hi, C.c_void_p(w.ctypes.data))
    return rc, w


# ---------------------------------------------------------------- host entries
@pytest.mark.parametrize("n_mels,n_bins,empty", [(80, 513, 0), (7, 1025, 0), (128, 257, 1)])
def test_mel_matrix_matches_the_oracle(seld_lib, n_mels, n_bins, empty):
    rc, w = lib_mel(seld_lib, n_mels, n_bins, D.SR)
    ref = D.mel_matrix(n_mels, n_bins, D.SR)
    assert rc == 0 and w.dtype == np.float32
    assert np.abs(w - ref).max() <= 1e-6 * ref.max()
    assert int((w.max(0) == 0).sum()) == int((ref.max(0) == 0).sum()) == empty
    assert np.array_equal(w != 0, ref != 0)      # the sparse table's supports are the oracle's


def test_python_mel_scale_is_the_library_matrix(seld_lib):
    from seld_amd import vad_dataloader as L
    assert np.array_equal(L.get_mel_scale(1024, 80, 16000), lib_mel(seld_lib, 80, 513, 16000)[1])


@pytest.mark.parametrize("n,frames", [(1023, 0), (1024, 1), (1535, 1), (1536, 2)])
def test_frame_counts(seld_lib, n, frames):
    assert seld_lib.seld_vad_feat_frames(1024, n) == frames == D.n_frames(1024, n)
    assert D.n_frames(1024, n) == (D.magnitudes(np.zeros(n), 1024).shape[0] if n >= 1024 else 0)      # torch.stft(center=False) frames alike


def test_case_files_have_the_frames_the_cases_name():
    assert [D.n_frames(1024, n) for n in D.FILE_LENGTHS] == [1, 1, 2, 6, 3]
    for n_fft, _, lengths, _ in D.SIZE_CASES.values():
        assert 1 in [D.n_frames(n_fft, n) for n in lengths]


# ---------------------------------------------------------------- oracle pins
def test_oracle_mel_pins():
    w = D.mel_matrix(80, 513, D.SR)
    assert not w[0].any()
    assert ((w > 0).sum(0) >= 2).all()
    k = np.arange(513)
    for m in range(80):      # every support is one contiguous run: what the sparse table relies on
        nz = k[w[:, m] > 0]
        assert nz[-1] - nz[0] + 1 == len(nz)
    assert int((D.mel_matrix(7, 1025, D.SR) > 0).sum(0).max()) == 520
    assert abs(float(D.hz_to_mel(700.0 * (np.e - 1.0))) - 1127.0) < 1e-9 and float(D.hz_to_mel(0.0)) == 0.0      # mel(f) = 1127 ln(1 + f / 700)


def test_oracle_threshold_pins():
    t = D.thresholds(200)
    assert t.dtype == np.float32 and len(t) == 201 and (np.diff(t) > 0).all()
    assert t[0] == np.float32(-1e-7) and t[-1] == np.float32(1.0 + 1e-7) and np.float32(0.5) in t
    assert np.array_equal(np.setdiff1d(t, D.auc_thresholds(200)), np.float32([0.5]))
    assert D.auc_thresholds(200)[1] == np.float32(1 / 199) and D.auc_thresholds(200)[-2] == np.float32(198 / 199)
    from seld_amd import vad_metrics as M
    assert np.array_equal(M.threshold_table(200), t)


def test_oracle_auc_pins():
    y = np.float32([0, 0, 1, 1, 0, 1])
    sep = D.metrics(np.float32([0.1, 0.2, 0.8, 0.9, 0.3, 0.7]), y)
    assert sep["auc"] == 1.0 and sep["precision"] == 1.0 and sep["recall"] == 1.0 and sep["binary_accuracy"] == 1.0
    const = D.metrics(np.full(6, 0.3, np.float32), y)
    assert const["auc"] == 0.5 and const["precision"] == 0.0 and const["recall"] == 0.0 and const["f1"] == 0.0 and const["binary_accuracy"] == 0.5
    assert D.metrics(np.float32([0.6, 0.4]), np.float32([0, 0]))["auc"] == 0.0      # no positive: every ratio with a zero denominator is 0


def test_python_results_equal_the_oracle_on_the_same_counts():
    from seld_amd import vad_metrics as M
    for labels in ("zeros", "ones", "mixed"):
        p, y = D.score_inputs(3001, labels, seed=3)
        c = D.bucket_counts(p, y, D.thresholds())
        got, ref = M.results_from_counts(c), D.metrics_from_counts(c, D.thresholds())
        assert c.sum() == 3001 and set(got) == {"auc", "precision", "recall", "f1", "binary_accuracy"}
        for k in ref:
            assert abs(got[k] - ref[k]) <= 1e-9, (labels, k)


def test_oracle_label_rounding_is_half_to_even():
    half = np.concatenate([np.ones(512), np.zeros(512)])
    assert D.frame_labels(half, 1024).tolist() == [0.0]
    assert D.frame_labels(np.concatenate([np.full(512, 1.0), np.full(512, 2.0)]), 1024).tolist() == [2.0]
    assert D.frame_labels(np.concatenate([np.ones(513), np.zeros(511)]), 1024).tolist() == [1.0]


# ---------------------------------------------------------------- refusals
def refusal_checks(lib):
    """every refusal of the new C entries: made before anything is enqueued, so the dummy non-NULL pointers are never read.  Shared with
    tests/test_vad_data_gpu.py, which runs it beside a live device."""
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    offs = (C.c_int32 * 65)(*range(65))
    bad0, unsorted = (C.c_int32 * 3)(1, 2, 3), (C.c_int32 * 3)(0, 2, 1)
    h = C.c_void_p()
    # create: scalars first, then sizes — all before any device call
    for sr, n_fft, n_mels, dev, rc in ((0, 1024, 80, 0, INVALID), (16000, 0, 80, 0, INVALID), (16000, 1024, 0, 0, INVALID), (16000, 1024, 80, -1, INVALID),
                                       (16000, 256, 80, 0, UNSUPPORTED), (16000, 4096, 80, 0, UNSUPPORTED), (16000, 1000, 80, 0, UNSUPPORTED),
                                       (16000, 1024, 257, 0, UNSUPPORTED)):
        assert lib.seld_vad_feat_create(sr, n_fft, n_mels, dev, C.byref(h)) == rc and not h.value, (sr, n_fft, n_mels, dev)
    assert lib.seld_vad_feat_create(16000, 1024, 80, 0, None) == INVALID
    lib.seld_vad_feat_destroy(None)
    # mel matrix
    for a in ((0, 513, 16000, 0.0, 8000.0, p), (80, 1, 16000, 0.0, 8000.0, p), (80, 513, 0, 0.0, 8000.0, p), (80, 513, 16000, -1.0, 8000.0, p),
              (80, 513, 16000, 8000.0, 8000.0, p), (80, 513, 16000, 0.0, 8000.5, p), (80, 513, 16000, 0.0, 8000.0, None),
              (80, 513, 16000, float("nan"), 8000.0, p)):
        assert lib.seld_vad_mel_matrix_host(*a) == INVALID, a[:5]
    assert lib.seld_vad_feat_frames(1024, -5) == 0 and lib.seld_vad_feat_frames(0, 100) == 0
    # extract: the handle comes first
    assert lib.seld_vad_feat_extract(None, p, p, p, 1, 2048, 3, 1, 1, p, None) == INVALID
    # frame labels
    ok = [p, p, p, 1, 2048, 3, 1024, p, None]
    for i, v in ((0, None), (1, None), (2, None), (7, None), (3, 0), (4, 1023), (5, 0), (6, 0), (6, 1023)):
        a = list(ok)
        a[i] = v
        assert lib.seld_vad_frame_labels(*a) == INVALID, (i, v)
    # gather
    ok = [p, p, p, offs, 7, 4, 80, 13, p, p, None]
    for i, v in ((0, None), (1, None), (2, None), (3, None), (8, None), (9, None), (4, 0), (5, 0), (6, 0), (7, 0), (3, bad0), (3, unsorted)):
        a = list(ok)
        a[i] = v
        if i == 3 and v is not None:
            a[4] = 3
        assert lib.seld_vad_gather(*a) == INVALID, (i,)
    a = list(ok)
    a[4] = 65
    assert lib.seld_vad_gather(*a) == UNSUPPORTED
    big = 0x7fffffff
    for B, Wn, Dm in ((big, 7, 80), (big, 64, big)):      # B Wn D beyond 0x7fffffff * 256 threads; the second product does not fit 64 bits
        a = list(ok)
        a[4], a[5], a[6] = Wn, B, Dm
        assert lib.seld_vad_gather(*a) == UNSUPPORTED, (B, Wn, Dm)
    a = [p, p, p, 1, 2048, big * 4 + 1, 1024, p, None]      # more frames than a grid of four-frame workgroups holds
    assert lib.seld_vad_frame_labels(*a) == UNSUPPORTED
    # scorer
    ok = [p, p, 10, p, 201, p, None]
    for i, v in ((0, None), (1, None), (3, None), (5, None), (2, 0), (4, 0)):
        a = list(ok)
        a[i] = v
        assert lib.seld_vad_score_update(*a) == INVALID, (i, v)
    a = list(ok)
    a[4] = 1025
    assert lib.seld_vad_score_update(*a) == UNSUPPORTED
    a = list(ok)
    a[2] = (1 << 40) + 1      # a workgroup's 32-bit buckets hold n / 1024 elements
    assert lib.seld_vad_score_update(*a) == UNSUPPORTED


def test_refusals_come_before_any_launch(seld_lib):
    refusal_checks(seld_lib)


def test_abi_declares_exports_and_binds_the_new_entries(seld_lib):
    from seld_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "seld_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name + "(" in hdr and name in _lib.SIGNATURES and hasattr(seld_lib, name)
    assert "vad_feat.hip" in open(os.path.join(ROOT, "seld_amd", "csrc", "Makefile")).read()


def _write_wav(path, data, width=2, channels=1, sr=16000):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(channels), w.setsampwidth(width), w.setframerate(sr)
        w.writeframes(data)


def test_wav_reader_scales_like_decode_wav_and_refuses_other_formats(tmp_path):
    from seld_amd import vad_dataloader as L
    pcm = np.array([0, 1, -1, 32767, -32768, 12345], "<i2")
    _write_wav(tmp_path / "a.wav", pcm.tobytes(), sr=8000)
    x, sr = L.read_wav(tmp_path / "a.wav")
    assert sr == 8000 and x.dtype == np.float32 and np.array_equal(x, pcm.astype(np.float32) / np.float32(32768.0))
    _write_wav(tmp_path / "b.wav", np.zeros(10, np.uint8).tobytes(), width=1)
    _write_wav(tmp_path / "c.wav", np.zeros(12, np.uint8).tobytes(), width=3)
    _write_wav(tmp_path / "d.wav", np.zeros(8, "<i2").tobytes(), channels=2)
    for n in "bcd":
        with pytest.raises(ValueError):
            L.read_wav(tmp_path / f"{n}.wav")
        with pytest.raises(ValueError):
            L.load_wav_and_extract_feat(tmp_path / f"{n}.wav")


def test_loader_refusals_need_no_device(tmp_path):
    from seld_amd import train_vad_baseline as T, vad_dataloader as L, vad_metrics as M
    long, short = np.zeros(1024 * 30, np.float32), np.zeros(1023, np.float32)
    win = [-19, -10, -1, 0, 1, 10, 19]
    with pytest.raises(ValueError):      # shorter than n_fft
        L.load_wav_and_extract_feat(short)
    with pytest.raises(ValueError):
        L.load_label(short)
    with pytest.raises(ValueError):
        L.get_vad_dataset([long, short], [long, short], win)
    with pytest.raises(ValueError):      # 39 frames > 38 are needed: 1024 * 20 samples give 39, 1024 * 19.5 give 38
        L.get_vad_dataset([np.zeros(1024 + 512 * 37, np.float32)], [np.zeros(1024 + 512 * 37, np.float32)], win)
    with pytest.raises(ValueError):      # label and wav lengths differ
        L.get_vad_dataset([long], [long[:-1]], win)
    with pytest.raises(ValueError):
        L.get_vad_dataset([long], [long, long], win)
    _write_wav(tmp_path / "r8k.wav", np.zeros(1024 * 30, "<i2").tobytes(), sr=8000)
    with pytest.raises(ValueError, match="8000 Hz"):      # a wav at another rate than the dataset's sr
        L.get_vad_dataset([str(tmp_path / "r8k.wav")], [long], win)
    for kw in ({"n_fft": 256}, {"n_fft": 1000}, {"n_mels": 0}, {"n_mels": 257}):
        with pytest.raises(ValueError):
            L.load_wav_and_extract_feat(long, **kw)
    with pytest.raises(ValueError):      # a mel matrix that is not get_mel_scale's
        L.load_wav_and_extract_feat(long, mel_scale=np.ones((513, 80), np.float32))
    with pytest.raises(ValueError):
        L.load_wav_and_extract_feat(long, mel_scale=L.get_mel_scale(1024, 80, 8000), sr=16000)
    feat, lab = np.zeros((38, 80, 1), np.float32), np.zeros(38, np.float32)
    with pytest.raises(ValueError):      # n_frames <= max(window)
        L.get_vad_dataset_from_pairs([(feat, lab)], win)
    with pytest.raises(ValueError):
        L.get_vad_dataset_from_pairs([(np.zeros((40, 80, 1), np.float32), np.zeros(39, np.float32))], win)
    with pytest.raises(ValueError):
        T.prepare_dataset([(feat, lab)], win, 4)
    for bad in (1, 1024, 2.5):
        with pytest.raises(ValueError):
            M.threshold_table(bad)
    if not torch.cuda.is_available():    # and what passes every check names the missing device instead of falling back
        with pytest.raises(RuntimeError):
            L.load_wav_and_extract_feat(long)
        with pytest.raises(RuntimeError):
            M.VADMetrics()


def test_file_walk_pairs_names(tmp_path):
    from seld_amd import vad_dataloader as L
    (tmp_path / "wav" / "sub").mkdir(parents=True)
    for n in ("wav/b.wav", "wav/sub/a.wav", "wav/skip.txt"):
        (tmp_path / n).write_bytes(b"")
    wavs, labels = L.extract_vad_fnames(str(tmp_path / "wav"), "lab")
    assert [os.path.relpath(w, tmp_path) for w in wavs] == ["wav/b.wav", "wav/sub/a.wav"]
    assert labels == [os.path.join("lab", "b.npy"), os.path.join("lab", "a.npy")]


# ---------------------------------------------------------------- fp32 room under the GPU bar
def _room(files, n_fft, n_mels, pairs):
    worst = 0.0
    for x in files:
        for lm, nz in pairs:
            a = D.front_end(x, n_fft, n_mels, D.SR, lm, nz, torch.float32)
            b = D.front_end(x, n_fft, n_mels, D.SR, lm, nz)
            worst = max(worst, rel_err(a, b))
    return worst


def test_fp32_room_of_the_default_case():
    """measured: at most 8.3e-7 on the broadband cases (this one and the three other sizes)"""
    e = _room(D.noisy_files(D.FILE_LENGTHS, D.FILE_GAINS), 1024, 80, D.FLAG_PAIRS)
    print(f"[room] default {e:.3e}")
    assert e <= REL_TOL / 2


@pytest.mark.parametrize("name", sorted(D.SIZE_CASES))
def test_fp32_room_of_the_other_sizes(name):
    n_fft, n_mels, lengths, gains = D.SIZE_CASES[name]
    e = _room(D.noisy_files(lengths, gains, seed=2), n_fft, n_mels, D.FLAG_PAIRS)
    print(f"[room] {name} {e:.3e}")
    assert e <= REL_TOL / 2


def test_fp32_room_of_the_pure_tone_holds_before_the_log_only():
    """a pure tone leaves most bands at the transform's rounding floor: their logs are noise in fp32 (measured 2e-2 .. 5e-2 of the maximum), so
    the GPU test compares this case before the log only, where plain fp32 stays far inside the bar"""
    x = D.tone_file()
    assert _room([x], 1024, 80, ((0, 0),)) <= REL_TOL / 2
    assert _room([x], 1024, 80, ((1, 0), (1, 1))) > REL_TOL


def test_silent_file_is_all_nan_in_the_oracle_as_in_the_reference_arithmetic():
    z = np.zeros(2048, np.float32)
    assert np.isnan(D.front_end(z, 1024, 80, D.SR, True, True)).all()
    assert np.isnan(D.front_end(z, 1024, 80, D.SR, False, True)).all()
    assert np.isneginf(D.front_end(z, 1024, 80, D.SR, True, False)).all()
