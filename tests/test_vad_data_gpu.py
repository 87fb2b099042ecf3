"""The voice-activity data path on the device: the seld_vad_feat_* / _frame_labels / _gather / _score_update entries (seld_amd/csrc/vad_feat.hip)
through the C ABI, then seld_amd/vad_dataloader.py, vad_metrics.py and train_vad_baseline.py, against the fp64 restatement
tests/vad_data_oracle.py.  Floating-point outputs are judged at the project's bar (helpers.check: max|d| / max|ref| <= 1e-4), every FILE against
its own oracle rows so that extrema leaking between files show; labels, gathers and counters are compared exactly.  tests/test_vad_data_cpu.py
asserts, on the same cases, that plain fp32 stays within half that bar of fp64 — and that the pure tone does not once the log is taken, which
is why that case is compared before the log only.

Outputs are written into NaN-filled allocations with a band behind them that must still be NaN after the call (tests/test_vad_gpu.py's _Out)."""
import ctypes as C
import functools
import os
import wave

import numpy as np
import pytest
import torch

import vad_data_oracle as D
import vad_oracle as V
from helpers import check, ptr
from test_vad_data_cpu import refusal_checks
from test_vad_gpu import GUARD, _Out, _stream, bits

pytestmark = pytest.mark.gpu


def _i64(a):
    return torch.as_tensor(np.asarray(a, np.int64)).cuda()


def _f32(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.float32)).cuda()


@functools.lru_cache(maxsize=None)
def _handle(n_fft, n_mels):
    from seld_amd import _lib
    h = C.c_void_p()
    assert _lib.load().seld_vad_feat_create(D.SR, n_fft, n_mels, torch.cuda.current_device(), C.byref(h)) == 0 and h.value
    return h


def extract(lib, files, n_fft, n_mels, logmel, normalize):
    """-> (device [total_frames, n_mels], frame_starts) through the C ABI with a guarded output"""
    wav, ss = D.pack(files)
    fs = D.frame_starts(n_fft, [len(f) for f in files])
    out = _Out(int(fs[-1]) * n_mels)
    wav_d, ss_d, fs_d = _f32(wav), _i64(ss), _i64(fs)
    rc = lib.seld_vad_feat_extract(_handle(n_fft, n_mels), ptr(wav_d), ptr(ss_d), ptr(fs_d), len(files), int(ss[-1]), int(fs[-1]), int(logmel),
                                   int(normalize), out.ptr(), _stream())
    assert rc == 0
    torch.cuda.synchronize()
    return out.get(int(fs[-1]), n_mels), fs


@functools.lru_cache(maxsize=None)
def default_files():
    return tuple(D.noisy_files(D.FILE_LENGTHS, D.FILE_GAINS))


@functools.lru_cache(maxsize=None)
def default_refs(logmel, normalize):
    return tuple(D.front_end(x, 1024, 80, D.SR, logmel, normalize) for x in default_files())


def _judge(name, got, fs, refs):
    worst = 0.0
    for i, ref in enumerate(refs):
        rows = got[int(fs[i]):int(fs[i + 1])].cpu().numpy()
        assert rows.shape == ref.shape
        worst = max(worst, check(f"{name} file {i}", rows, ref))
    return worst


# ---------------------------------------------------------------- 1 - 5: the front end
@pytest.mark.parametrize("logmel,normalize", D.FLAG_PAIRS)
def test_front_end_default_sizes(seld_lib, logmel, normalize):
    got, fs = extract(seld_lib, default_files(), 1024, 80, logmel, normalize)
    assert fs.tolist() == [0, 1, 2, 4, 10, 13]
    _judge(f"feat 1024x80 ({logmel},{normalize})", got, fs, default_refs(logmel, normalize))


@pytest.mark.parametrize("logmel,normalize", [(0, 0), (1, 1)])
def test_files_do_not_see_each_other(seld_lib, logmel, normalize):
    files = default_files()
    got, fs = extract(seld_lib, files, 1024, 80, logmel, normalize)
    for i, x in enumerate(files):
        alone, _ = extract(seld_lib, [x], 1024, 80, logmel, normalize)
        assert torch.equal(bits(alone), bits(got[int(fs[i]):int(fs[i + 1])])), f"file {i}"


@pytest.mark.parametrize("name", sorted(D.SIZE_CASES))
def test_front_end_other_sizes(seld_lib, name):
    n_fft, n_mels, lengths, gains = D.SIZE_CASES[name]
    files = D.noisy_files(lengths, gains, seed=2)
    empty = np.flatnonzero(D.mel_matrix(n_mels, n_fft // 2 + 1, D.SR).max(0) == 0)
    assert len(empty) == (1 if name == "512x128" else 0)
    for logmel, normalize in D.FLAG_PAIRS:
        got, fs = extract(seld_lib, files, n_fft, n_mels, logmel, normalize)
        _judge(f"feat {name} ({logmel},{normalize})", got, fs, [D.front_end(x, n_fft, n_mels, D.SR, logmel, normalize) for x in files])
        if len(empty) and logmel == normalize:      # raw, and after the log and the normalisation: the empty filter's column is exactly 0
            assert not got[:, int(empty[0])].cpu().numpy().any()


def test_pure_tone_before_the_log(seld_lib):
    x = D.tone_file()
    got, fs = extract(seld_lib, [x], 1024, 80, 0, 0)
    _judge("feat tone (0,0)", got, fs, [D.front_end(x, 1024, 80, D.SR, False, False)])


def test_silent_file_is_all_nan_and_its_neighbours_are_untouched(seld_lib):
    a, b = D.noisy_files((2048, 3000), (1.0, 0.2), seed=5)
    files = [a, np.zeros(1536, np.float32), b]
    got, fs = extract(seld_lib, files, 1024, 80, 1, 1)
    assert fs.tolist() == [0, 3, 5, 9]
    assert bool(torch.isnan(got[3:5]).all())
    for x, (r0, r1) in ((a, (0, 3)), (b, (5, 9))):
        alone, _ = extract(seld_lib, [x], 1024, 80, 1, 1)
        assert torch.equal(bits(alone), bits(got[r0:r1])) and bool(torch.isfinite(alone).all())
    raw, _ = extract(seld_lib, files, 1024, 80, 0, 0)
    assert not raw[3:5].cpu().numpy().any()
    logged, _ = extract(seld_lib, files, 1024, 80, 1, 0)
    assert bool(torch.isneginf(logged[3:5]).all())      # log(min(max(0, 1e-8), 0)) = log 0, the literal arithmetic


def test_handle_create_and_destroy(seld_lib):
    h = C.c_void_p()
    assert seld_lib.seld_vad_feat_create(8000, 512, 1, torch.cuda.current_device(), C.byref(h)) == 0 and h.value
    seld_lib.seld_vad_feat_destroy(h)
    assert seld_lib.seld_vad_feat_create(16000, 1024, 80, 1 << 20, C.byref(h)) == -3 and not h.value      # no such device: SELD_ERR_HIP
    refusal_checks(seld_lib)


def test_extract_refusals_with_a_live_handle(seld_lib):
    """every refusal of seld_vad_feat_extract behind the handle check, on real buffers: nothing is enqueued, so the NaN-filled output keeps its bits.
    total_samples < n_fft is the one the frame-start clamp rests on"""
    h = _handle(1024, 80)
    wav_d, ss_d, fs_d = _f32(np.ones(2048)), _i64([0, 2048]), _i64([0, 3])
    out = _Out(3 * 80)
    ok = [h, ptr(wav_d), ptr(ss_d), ptr(fs_d), 1, 2048, 3, 1, 1, out.ptr(), _stream()]
    for i, v in ((1, None), (2, None), (3, None), (9, None), (4, 0), (4, -1), (6, 0), (6, -3), (5, 1023), (5, 0), (5, -1)):
        a = list(ok)
        a[i] = v
        assert seld_lib.seld_vad_feat_extract(*a) == -1, (i, v)
    for frames, rc in (((1 << 40) // 80 + 1, -2), (1 << 62, -2)):      # total_frames n_mels beyond 2^40 elements
        a = list(ok)
        a[6] = frames
        assert seld_lib.seld_vad_feat_extract(*a) == rc, frames
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.get(3, 80)).all())
    assert seld_lib.seld_vad_feat_extract(*ok) == 0      # and the same arguments, unchanged, run
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out.get(3, 80)).all())


# ---------------------------------------------------------------- 6: frame labels
def frame_labels(lib, labels, n_fft):
    lab, ss = D.pack(labels)
    fs = D.frame_starts(n_fft, [len(a) for a in labels])
    out = _Out(int(fs[-1]))
    lab_d, ss_d, fs_d = _f32(lab), _i64(ss), _i64(fs)
    assert lib.seld_vad_frame_labels(ptr(lab_d), ptr(ss_d), ptr(fs_d), len(labels), int(ss[-1]), int(fs[-1]), n_fft, out.ptr(), _stream()) == 0
    torch.cuda.synchronize()
    return out.get(int(fs[-1])).cpu().numpy()


def test_frame_labels(seld_lib):
    labels = D.binary_labels(D.FILE_LENGTHS)
    got = frame_labels(seld_lib, labels, 1024)
    ref = np.concatenate([D.frame_labels(a, 1024) for a in labels])
    assert got.shape == (13,) and np.array_equal(got, ref) and 0 < ref.sum() < 13
    half = np.concatenate([np.ones(512), np.zeros(512)]).astype(np.float32)            # the sum is exactly n_fft / 2: 0.5 rounds to 0
    one_two = np.concatenate([np.ones(512), np.full(512, 2.0)]).astype(np.float32)      # mean 1.5 rounds to 2
    more = np.concatenate([np.ones(513), np.zeros(511)]).astype(np.float32)
    assert frame_labels(seld_lib, [half, one_two, more], 1024).tolist() == [0.0, 2.0, 1.0]
    assert frame_labels(seld_lib, [half[::2].copy(), one_two[::2].copy()], 512).tolist() == [0.0, 2.0]


# ---------------------------------------------------------------- 7: window batches
@pytest.mark.parametrize("Dm", [80, 7, 1])
@pytest.mark.parametrize("window", [D.REF_WINDOW, [0, 1, 2]], ids=["ref", "range3"])
def test_gather(seld_lib, Dm, window):
    rng = np.random.default_rng(Dm)
    total, width, Wn = 301, max(window), len(window)
    feat, y = rng.standard_normal((total, Dm)).astype(np.float32), rng.integers(0, 2, total).astype(np.float32)
    feat_d, y_d = _f32(feat), _f32(y)
    offs = (C.c_int32 * Wn)(*window)
    for B in (1, 5, 257):
        pos = rng.integers(0, total - width, B).astype(np.int64)
        pos[-1] = total - 1 - width                       # the last feasible row of the corpus
        pos_d = _i64(pos)
        xo, yo = _Out(B * Wn * Dm), _Out(B * Wn)
        assert seld_lib.seld_vad_gather(ptr(feat_d), ptr(y_d), ptr(pos_d), offs, Wn, B, Dm, total, xo.ptr(), yo.ptr(), _stream()) == 0
        torch.cuda.synchronize()
        rx, ry = D.gather(feat, y, pos, window)
        assert np.array_equal(xo.get(B, Wn, Dm).cpu().numpy().view(np.int32), rx.view(np.int32)), (B,)
        assert np.array_equal(yo.get(B, Wn).cpu().numpy(), ry), (B,)
    # rows are clamped into the corpus: positions outside it read its first / last row
    pos = np.int64([-5, total + 3])
    pos_d = _i64(pos)
    xo, yo = _Out(2 * Wn * Dm), _Out(2 * Wn)
    assert seld_lib.seld_vad_gather(ptr(feat_d), ptr(y_d), ptr(pos_d), offs, Wn, 2, Dm, total, xo.ptr(), yo.ptr(), _stream()) == 0
    torch.cuda.synchronize()
    rx, ry = D.gather(feat, y, pos, window)
    assert np.array_equal(xo.get(2, Wn, Dm).cpu().numpy(), rx) and np.array_equal(yo.get(2, Wn).cpu().numpy(), ry)


# ---------------------------------------------------------------- 8: the scorer
@pytest.mark.parametrize("n", [1, 255, 257, 70001])
@pytest.mark.parametrize("labels", ["zeros", "ones", "mixed"])
def test_score_counters_and_results(seld_lib, n, labels):
    from seld_amd import vad_metrics as M
    thr = D.thresholds()
    NT = len(thr)
    thr_d = _f32(thr)
    buf = torch.full((2 * (NT + 1) + GUARD,), -7, dtype=torch.int64, device="cuda")
    buf[:2 * (NT + 1)] = 0
    ref = np.zeros((NT + 1, 2), np.int64)
    for seed in (0, 1):                                    # two updates into the same counters
        p, y = D.score_inputs(n, labels, seed=seed + 10 * n)
        p_d, y_d = _f32(p), _f32(y)
        assert seld_lib.seld_vad_score_update(ptr(p_d), ptr(y_d), n, ptr(thr_d), NT, C.c_void_p(buf.data_ptr()), _stream()) == 0
        ref += D.bucket_counts(p, y, thr)
    torch.cuda.synchronize()
    assert bool((buf[2 * (NT + 1):] == -7).all())
    got = buf[:2 * (NT + 1)].cpu().numpy().reshape(NT + 1, 2)
    assert got.sum() == 2 * n and np.array_equal(got, ref)
    a, b = M.results_from_counts(got), D.metrics_from_counts(ref, thr)
    for k in b:
        assert abs(a[k] - b[k]) <= 1e-9, k
    if n == 70001:
        assert ref[0].sum() >= 2      # the NaNs (and -1e-7's own value) sit in bucket 0


def test_vad_metrics_class_accumulates_and_resets():
    from seld_amd import vad_metrics as M
    m = M.VADMetrics()
    parts = [D.score_inputs(1000, "mixed", seed=s) for s in (0, 1)]
    for p, y in parts:
        m.update_state(_f32(y).reshape(10, 100), _f32(p).reshape(100, 10, 1))
    ref = D.metrics(np.concatenate([p for p, _ in parts]), np.concatenate([y for _, y in parts]))
    got = m.result()
    for k in ref:
        assert abs(got[k] - ref[k]) <= 1e-9, k
    assert 0.3 < got["auc"] < 0.7
    m.reset_states()
    assert int(m.counts.sum()) == 0
    with pytest.raises(ValueError):
        m.update_state(torch.zeros(3), torch.zeros(4))


# ---------------------------------------------------------------- 9: the Python path
def _corpus(tmp_path):
    rng = np.random.default_rng(7)
    lengths = (1024 + 512 * 44, 1024 + 512 * 59)            # 45 and 60 frames
    wavs, labs, pcms = [], [], []
    for i, (x, lab) in enumerate(zip(D.noisy_files(lengths, (0.8, 0.3), seed=9), D.binary_labels(lengths, seed=4))):
        pcm = np.clip(np.round(x * 32768.0), -32768, 32767).astype("<i2")
        with wave.open(str(tmp_path / f"u{i}.wav"), "wb") as w:
            w.setnchannels(1), w.setsampwidth(2), w.setframerate(D.SR)
            w.writeframes(pcm.tobytes())
        np.save(tmp_path / f"u{i}.npy", lab)
        wavs.append(str(tmp_path / f"u{i}.wav")), labs.append(str(tmp_path / f"u{i}.npy")), pcms.append(pcm.astype(np.float64) / 32768.0)
    return wavs, labs, pcms, [np.load(p) for p in labs], rng


def test_python_path_dataset_batches_training_and_evaluation(tmp_path):
    from seld_amd import train_vad_baseline as T, vad, vad_dataloader as L, vad_metrics as M
    wavs, labs, pcms, labels, rng = _corpus(tmp_path)
    window = [-19, -10, -1, 0, 1, 10, 19]
    ds = L.get_vad_dataset(wavs, labs, window, mel_scale=None)
    refs = [D.front_end(x, 1024, 80, D.SR, True, True) for x in pcms]
    ref_y = [D.frame_labels(a, 1024) for a in labels]
    assert ds.frame_starts.tolist() == [0, 45, 105] and tuple(ds.feats.shape) == (105, 80, 1) and ds.window.tolist() == D.REF_WINDOW
    _judge("dataset features", ds.feats[:, :, 0], ds.frame_starts, refs)
    assert np.array_equal(ds.labels.cpu().numpy(), np.concatenate(ref_y))
    # the single-file loaders give the same rows
    f0, y0 = L.extract_feat_label(wavs[0], labs[0], mel_scale=L.get_mel_scale(1024, 80, D.SR))
    assert tuple(f0.shape) == (45, 80, 1) and torch.equal(bits(f0), bits(ds.feats[:45])) and torch.equal(y0, ds.labels[:45])
    # batches with given draws: two passes over two utterances, batch 3 -> 3 + 1 windows
    draws = np.int64([0, 21, 6, 13])                       # 45 - 38 = 7 and 60 - 38 = 22 offsets are feasible
    got = list(ds.batches(3, n_repeat=2, draws=draws))
    assert [tuple(x.shape) for x, _ in got] == [(3, 7, 80, 1), (1, 7, 80, 1)] and [tuple(y.shape) for _, y in got] == [(3, 7), (1, 7)]
    pos = np.int64([0, 45, 0, 45]) + draws
    rx, ry = D.gather(np.concatenate(refs), np.concatenate(ref_y), pos, D.REF_WINDOW)
    x_all, y_all = torch.cat([x for x, _ in got]), torch.cat([y for _, y in got])
    check("batch windows", x_all[..., 0].cpu().numpy(), rx)
    assert np.array_equal(y_all.cpu().numpy(), ry)
    bx, _ = D.gather(ds.feats.cpu().numpy(), ds.labels.cpu().numpy(), pos, D.REF_WINDOW)
    assert np.array_equal(x_all.cpu().numpy(), bx)
    for bad in ([0, 22, 0, 0], [7, 0, 0, 0], [0, 0, 0], [-1, 0, 0, 0]):
        with pytest.raises(ValueError):
            next(ds.batches(3, n_repeat=2, draws=bad))
    off = ds.draw(400, rng).reshape(400, 2)
    assert off.min() == 0 and off[:, 0].max() == 6 and off[:, 1].max() == 21
    shuffled = ds.positions(3, shuffle=True, rng=np.random.default_rng(0))
    assert sorted((shuffled[i:i + 2] >= 45).sum() for i in (0, 2, 4)) == [1, 1, 1]      # every pass holds each utterance once
    # three training steps, the checkpoint and its reload
    cfg = {"T": 2, "dropout_rate": 0.0}
    name = str(tmp_path / "vad_ckpt")
    trainset = T.prepare_dataset(ds, window, 4, train=True, n_repeat=6, rng=np.random.default_rng(1))
    valset = T.prepare_dataset(ds.pairs(), window, 4)
    assert len(list(trainset)) == 3
    model, hist = T.train_and_eval(cfg, [4, 7, 80, 1], trainset, valset, epochs=1, name=name)
    assert os.path.exists(name + ".npz") and len(hist["loss"]) == len(hist["val_auc"]) == 1 and np.isfinite(hist["loss"][0]) and 0.0 <= hist["val_auc"][0] <= 1.0
    w, s = model.get_weights()
    z = np.load(name + ".npz")
    for n_, o, sh in model.variables:
        assert np.array_equal(w[o:o + int(np.prod(sh))].reshape(sh), z[n_]), n_
    # evaluate_pairs against VADMetrics fed the oracle's windows_to_seq of the same model outputs
    pairs = ds.pairs()
    got = T.evaluate_pairs(model, pairs, window, 4)
    m = M.VADMetrics()
    for x, y in pairs:
        wins = vad.seq_to_windows(x, D.REF_WINDOW)
        outs = torch.cat([model(wins[i:i + 4])[0] for i in range(0, wins.shape[0], 4)]).cpu().numpy()
        seq = V.windows_to_seq(outs, D.REF_WINDOW)
        assert seq.shape == (len(y), 1)
        m.update_state(y, torch.as_tensor(seq.astype(np.float32)))
    ref = m.result()
    for k in ref:
        assert abs(got[k] - ref[k]) <= 1e-9, k
    model.close()
