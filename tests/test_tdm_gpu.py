"""Time-domain mixing on the device against tests/tdm_oracle.py, bit for bit: seld_aug_tdm_labels and seld_aug_tdm_mix through the C ABI on the
hand-built plans of tests/tdm_cases.py (what each plan is there for: its docstring, checked by tests/test_tdm_cpu.py), data_loader.TDM_aug,
train.get_tdm_dataset and train.main's regeneration schedule.  Every plan is in range: the kernels' guards against a bad plan row are not
exercised here, the host validation in front of them is (tests/test_tdm_cpu.py)."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import tdm_cases as TC
import tdm_oracle as TO

pytestmark = pytest.mark.gpu


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a, dtype)).cuda()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _pack_labels(tdm_y):
    rows = np.array([t.shape[0] for t in tdm_y], np.int64)
    row0 = np.concatenate([[0], np.cumsum(rows)[:-1]]).astype(np.int64)
    return _dev(np.concatenate(tdm_y), np.float32), _dev(row0), _dev(rows)


def _pack_waves(tdm_x, front=0):
    """the blocks [C][n_k] one behind the other, behind `front` unused floats -> (bank_x, bank_s0 [n_cls + 1])"""
    s0 = front + np.concatenate([[0], np.cumsum([t.size for t in tdm_x])]).astype(np.int64)
    flat = np.concatenate([np.zeros(front, np.float32)] + [t.reshape(-1) for t in tdm_x])
    return _dev(flat, np.float32), _dev(s0)


def _run_labels(lib, y, tdm_y, plan, max_per_frame=TC.MAX_PER_FRAME):
    """-> (y', valid) as numpy, the whole valid tensor the kernel wrote"""
    B, T, W = y.shape
    K = plan.shape[1]
    ld = max(1, int(plan[..., 1].max())) if plan.size else 1
    yd, pd = _dev(y, np.float32), (_dev(plan, np.int32) if K else None)
    valid = torch.full((B, K, ld), -7.0, device="cuda")
    by, r0, rs = _pack_labels(tdm_y)
    rc = lib.seld_aug_tdm_labels(_p(yd), B, T, W, _p(by), _p(r0), _p(rs), len(tdm_y), _p(pd), K, max_per_frame, _p(valid) if K else None, ld, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return yd.cpu().numpy(), valid.cpu().numpy()


# ---------------------------------------------------------------- the labels kernel
def test_labels_kernel_on_the_hand_built_plans(seld_lib):
    y, plan, expect = TC.labels_case()
    tdm_x, tdm_y = TC.make_bank(TC.BANK_ROWS, TC.NC, 1, 1, seed=1)
    _, want_y, want_v = TO.tdm_aug(np.zeros((3, 1, TC.T), np.float32), y, tdm_x, tdm_y, plan, 1, TC.MAX_PER_FRAME)
    got_y, got_v = _run_labels(seld_lib, y, tdm_y, plan)
    np.testing.assert_array_equal(got_v, want_v)
    np.testing.assert_array_equal(got_y, want_y)
    for (b, k), v in expect.items():                           # and the vectors written out by hand
        np.testing.assert_array_equal(got_v[b, k, :len(v)], np.array(v, np.float32))


def test_labels_kernel_k0_and_shorter_plans(seld_lib):
    y, plan, _ = TC.labels_case()
    tdm_x, tdm_y = TC.make_bank(TC.BANK_ROWS, TC.NC, 1, 1, seed=1)
    got_y, got_v = _run_labels(seld_lib, y, tdm_y, plan[:, :0])
    np.testing.assert_array_equal(got_y, y)
    assert got_v.shape == (3, 0, 1)
    for K in (1, 3):                                           # a prefix of the plan: the later insertions change nothing before them
        _, want_y, want_v = TO.tdm_aug(np.zeros((3, 1, TC.T), np.float32), y, tdm_x, tdm_y, plan[:, :K], 1, TC.MAX_PER_FRAME)
        got_y, got_v = _run_labels(seld_lib, y, tdm_y, plan[:, :K])
        np.testing.assert_array_equal(got_v, want_v)
        np.testing.assert_array_equal(got_y, want_y)


def test_labels_kernel_more_frames_than_threads(seld_lib):
    y, plan, rows = TC.long_case()
    tdm_x, tdm_y = TC.make_bank(rows, TC.NC, 1, 1, seed=3)
    _, want_y, want_v = TO.tdm_aug(np.zeros((2, 1, 320), np.float32), y, tdm_x, tdm_y, plan, 1, TC.MAX_PER_FRAME)
    got_y, got_v = _run_labels(seld_lib, y, tdm_y, plan)
    assert want_v.shape == (2, 2, 300)
    np.testing.assert_array_equal(got_v, want_v)
    np.testing.assert_array_equal(got_y, want_y)


# ---------------------------------------------------------------- the mix kernel
MIX_FORMS = {                       # spf, offset of the x view in floats, unused floats in front of the bank blocks
    "float4": (8, 0, 0),
    "float4_scalar_bank": (8, 0, 2),        # the clips take float4 accesses, the bank's blocks start off a 16-byte boundary
    "scalar_spf6": (6, 0, 0),
    "scalar_unaligned": (8, 1, 0),
}


@pytest.mark.parametrize("in_place", [True, False], ids=["in_place", "out_of_place"])
@pytest.mark.parametrize("tail", [0, 5])
@pytest.mark.parametrize("Cn", [4, 1])
@pytest.mark.parametrize("form", list(MIX_FORMS))
def test_mix_kernel(seld_lib, form, Cn, tail, in_place):
    """the plans of the labels case; clips and bank carry random floats, so where insertions overlap in time (clip 0: k0-k2, clip 1: k3 over
    k0-k2, clip 2: k0-k2) the order of the adds shows in the bits"""
    spf, shift, front = MIX_FORMS[form]
    y, plan, _ = TC.labels_case()
    tdm_x, tdm_y = TC.make_bank(TC.BANK_ROWS, TC.NC, Cn, spf, seed=1, extra=0)
    N = TC.T * spf + tail
    x = TC.waves(3, Cn, N, seed=2)
    want_x, _, valid = TO.tdm_aug(x, y, tdm_x, tdm_y, plan, spf, TC.MAX_PER_FRAME)
    assert not np.array_equal(want_x, x)
    store = torch.zeros(x.size + shift + 4, device="cuda")
    xin = store[shift:shift + x.size].view(3, Cn, N)
    xin.copy_(_dev(x))
    assert xin.data_ptr() % 16 == (4 * shift) % 16
    xout = xin if in_place else torch.full_like(xin, -7.0)
    bx, s0 = _pack_waves(tdm_x, front)
    K, ld = plan.shape[1], valid.shape[2]
    d_plan, d_valid = _dev(plan, np.int32), _dev(valid)              # held until the kernel has run
    rc = seld_lib.seld_aug_tdm_mix(_p(xin), _p(xout), 3, Cn, N, TC.T, spf, _p(bx), _p(s0), len(tdm_x), _p(d_plan), K, _p(d_valid), ld, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    np.testing.assert_array_equal(xout.cpu().numpy(), want_x)
    if not in_place:
        np.testing.assert_array_equal(xin.cpu().numpy(), x)
    assert float(store[:shift].abs().sum()) == 0 and float(store[shift + x.size:].abs().sum()) == 0      # nothing next to the view was written


def test_mix_kernel_k0(seld_lib):
    """no insertion: in place nothing is enqueued, out of place the clips are copied"""
    x = _dev(TC.waves(2, 4, 85, seed=4))
    tdm_x, _ = TC.make_bank((3,), 1, 4, 8, seed=1)
    bx, s0 = _pack_waves(tdm_x)
    out = torch.full_like(x, -7.0)
    for dst in (x, out):
        assert seld_lib.seld_aug_tdm_mix(_p(x), _p(dst), 2, 4, 85, 10, 8, _p(bx), _p(s0), 1, None, 0, None, 1, _stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, x)


# ---------------------------------------------------------------- TDM_aug
def _device_args(n=4, T=40, spf=8, Cn=4, seed=0):
    rng = np.random.default_rng(seed)
    tdm_x, tdm_y = TC.make_bank(TC.BANK_ROWS, TC.NC, Cn, spf, seed=1, extra=5)
    y = np.stack([TC._labels(T, TC.NC, {int(rng.integers(3)): [(5, 12)], int(rng.integers(3)): [(20, 31)]}, seed + i) for i in range(n)])
    return TC.waves(n, Cn, T * spf, seed + 50), y, tdm_x, tdm_y


def test_tdm_aug_matches_the_oracle_and_its_seed():
    from seld_amd import data_loader as dl
    x, y, tdm_x, tdm_y = _device_args()
    kw = dict(sr=80, max_overlap_num=5, min_overlap_sec=0.5, max_overlap_sec=1)
    bank = dl.TdmBank(tdm_x, tdm_y, sr=80)
    runs = []
    for seed in (3, 3, 4):
        xd, yd = _dev(x), _dev(y)
        ox, oy, valid = dl.TDM_aug(xd, yd, bank, rng=np.random.default_rng(seed), return_valid=True, **kw)
        assert ox is xd and oy is yd                              # in place
        plan = dl.draw_tdm(np.random.default_rng(seed), 4, 40, TC.BANK_ROWS, 5, 5, 10)
        want_x, want_y, want_v = TO.tdm_aug(x, y, tdm_x, tdm_y, plan, 8, 2)
        np.testing.assert_array_equal(valid.cpu().numpy(), want_v)
        np.testing.assert_array_equal(oy.cpu().numpy(), want_y)
        np.testing.assert_array_equal(ox.cpu().numpy(), want_x)
        runs.append((ox.cpu().numpy(), oy.cpu().numpy()))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    assert not np.array_equal(runs[0][0], runs[2][0]) and not np.array_equal(runs[0][1], runs[2][1])


def test_tdm_aug_lists_draws_and_out():
    """the bank as the two lists, x as a list of clips, an explicit plan, and `out`"""
    from seld_amd import data_loader as dl
    x, y, tdm_x, tdm_y = _device_args(n=3)
    _, plan, _ = TC.labels_case()
    want_x, want_y, _ = TO.tdm_aug(x, y, tdm_x, tdm_y, plan, 8, 2)
    yd = _dev(y)
    ox, oy = dl.TDM_aug([_dev(c) for c in x], yd, tdm_x, tdm_y, sr=80, draws=plan)
    np.testing.assert_array_equal(ox.cpu().numpy(), want_x)
    np.testing.assert_array_equal(oy.cpu().numpy(), want_y)
    xd, yd, out = _dev(x), _dev(y), torch.empty(x.shape, device="cuda")
    ox, _ = dl.TDM_aug(xd, yd, tdm_x, tdm_y, sr=80, draws=plan, out=out)
    assert ox is out
    np.testing.assert_array_equal(out.cpu().numpy(), want_x)
    np.testing.assert_array_equal(xd.cpu().numpy(), x)
    with pytest.raises(ValueError):
        dl.TDM_aug(xd[:, :, :-1].contiguous(), yd, tdm_x, tdm_y, sr=80, draws=plan)          # N < T * spf


# ---------------------------------------------------------------- get_tdm_dataset and main
SR, SPF, T_CLIP = 24000, 2400, 20
SYN_ROWS = (11, 14)          # label frames of the synthetic bank's two tracks: longer than the 9 frames train.main's first setting can draw


class _Config:
    batch, loop_time, use_tfm, use_acs, time_mask_size, freq_mask_size = 2, 1, False, False, 24, 16


@pytest.fixture(scope="module")
def synthetic():
    """4 clips of 20 label frames (48 000 samples at 24 kHz), 12 classes of labels, a 2-class bank"""
    rng = np.random.default_rng(0)
    nc = 12
    x = (0.1 * rng.standard_normal((4, 4, T_CLIP * SPF))).astype(np.float32)
    y = np.stack([TC._labels(T_CLIP, nc, {int(rng.integers(2, nc)): [(2, 9)], int(rng.integers(2, nc)): [(11, 17)]}, 20 + i) for i in range(4)])
    tdm_x, tdm_y = TC.make_bank(SYN_ROWS, nc, 4, SPF, seed=9, extra=11)
    tdm_x = [0.1 * t for t in tdm_x]
    return x, y, tdm_x, tdm_y


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def test_get_tdm_dataset_on_a_synthetic_source(synthetic):
    from seld_amd import data_loader as dl, train
    from seld_amd.feature_extractor import FeatureExtractor
    x, y, tdm_x, tdm_y = synthetic
    source = train.TdmSource(x, y, tdm_x, tdm_y)
    kw = dict(max_overlap_num=3, max_overlap_per_frame=2, min_overlap_sec=0.3, max_overlap_sec=0.8, source=source)
    # features: identity normalisation, so the windows ARE the extractor's output — the same kernel on the same bits
    F, Cf = 64, 7
    ds = train.get_tdm_dataset(_Config, rng=np.random.default_rng(5), norm=(np.zeros(F * Cf), np.ones(F * Cf)), chunk=3, **kw)
    plan = dl.draw_tdm(np.random.default_rng(5), 4, T_CLIP, SYN_ROWS, 3, 2, 8)
    np.testing.assert_array_equal(ds.tdm_plan, plan)
    want_x, want_y, valid = TO.tdm_aug(x, y, tdm_x, tdm_y, plan, SPF, 2)
    assert valid.sum() > 0 and not np.array_equal(want_x, x)
    fe = FeatureExtractor(SR, "foa", 64, n_fft=1024, win_length=1024, hop_length=480)
    feats = fe.batch(_dev(want_x))[:, :T_CLIP * 5].cpu().numpy()               # [4, 100, 64, 7]
    assert isinstance(ds, dl.SeldDataset) and ds.x.is_cuda and tuple(ds.x.shape) == (1, 300, 64, 7) and tuple(ds.y.shape) == (1, 60, 48)
    np.testing.assert_array_equal(ds.x.cpu().numpy(), feats.reshape(400, 64, 7)[:300].reshape(1, 300, 64, 7))
    np.testing.assert_array_equal(ds.y.cpu().numpy(), want_y.reshape(80, 48)[:60].reshape(1, 60, 48))
    np.testing.assert_array_equal(ds.tdm_labels.cpu().numpy(), want_y)
    np.testing.assert_array_equal(source.x.cpu().numpy(), x)                   # mixed out of place: the clean waves stay clean
    np.testing.assert_array_equal(source.y.cpu().numpy(), y)
    # the reference's normalisation (train.py:238): over the clip axis per (frame, freq, chan), population std, no eps
    ds2 = train.get_tdm_dataset(_Config, rng=np.random.default_rng(5), chunk=3, **kw)
    f64 = feats.astype(np.float64)
    mean, std = f64.mean(0), f64.std(0)
    assert std.min() > 0
    want = ((f64 - mean) / std).reshape(400, 64, 7)[:300].reshape(1, 300, 64, 7)
    got_mean, got_std = (t.cpu().numpy().reshape(100, 64, 7) for t in ds2.tdm_norm)
    print(f"[tdm] mean rel {_rel(got_mean, mean):.3e}  std rel {_rel(got_std, std):.3e}  normalised rel {_rel(ds2.x.cpu().numpy(), want):.3e}")
    assert _rel(got_mean, mean) < 1e-4 and _rel(got_std, std) < 1e-4
    assert _rel(ds2.x.cpu().numpy(), want) < 1e-4
    np.testing.assert_array_equal(ds2.y.cpu().numpy(), ds.y.cpu().numpy())
    np.testing.assert_array_equal(source.x.cpu().numpy(), x)                   # ... after the second call too
    assert source.regenerations == 2
    batches = list(ds2)
    assert len(batches) == 1 and tuple(batches[0][0].shape) == (1, 300, 64, 7) and tuple(batches[0][1][0].shape) == (1, 60, 12)
    # --use_tfm / --use_acs attach the device transforms of get_dataset
    cfg = type("C", (_Config,), dict(use_tfm=True, use_acs=True))
    assert len(train.get_tdm_dataset(cfg, rng=np.random.default_rng(5), **kw).device_transforms) == 3


def test_main_regenerates_on_schedule(tmp_path, seldnet_config, monkeypatch, synthetic):
    """train.main with --use_tdm for 2 epochs, tdm_epoch = 1: one training set per epoch, made from the one source"""
    from seld_amd import params, train
    x, y, tdm_x, tdm_y = synthetic
    root = tmp_path / "DCASE2021" / "feat_label"
    feat, lab = root / "foa_dev_norm", root / "foa_dev_label"
    feat.mkdir(parents=True), lab.mkdir(parents=True)
    rng = np.random.default_rng(0)
    for fold in (5, 6):
        name = f"fold{fold}_room1_mix000.npy"
        np.save(feat / name, rng.standard_normal((300, 64, 7)).astype(np.float32))
        sed = (rng.random((60, 12)) < 0.1).astype(np.float32)
        np.save(lab / name, np.concatenate([sed, np.zeros((60, 36), np.float32)], -1))
    mcd = tmp_path / "model_config"
    mcd.mkdir()
    (mcd / "seldnet.json").write_text(json.dumps(seldnet_config))
    monkeypatch.chdir(tmp_path)
    config, mc = params.get_param(["--name", "t", "--abspath", str(tmp_path) + "/", "--batch", "2", "--loop_time", "1", "--epoch", "2", "--use_tdm",
                                   "--tdm_epoch", "1", "--tdm_wav_path", "w", "--tdm_label_path", "l", "--tdm_bank_path", "b"], model_config_dir=str(mcd))
    source = train.TdmSource(x, y, tdm_x, tdm_y)
    model, hist = train.main((config, mc), tdm_source=source)
    assert len(hist) == 2 and all(np.isfinite(h["train"][0]) and np.isfinite(h["train"][1]) for h in hist)
    assert source.regenerations == 2
    np.testing.assert_array_equal(source.x.cpu().numpy(), x)
    bad = train.TdmSource(x, y.reshape(4, T_CLIP, 4, 12)[..., :10].reshape(4, T_CLIP, 40), tdm_x,
                          [t.reshape(-1, 4, 12)[..., :10].reshape(-1, 40) for t in tdm_y])
    with pytest.raises(ValueError, match="classes"):                          # 10 classes of labels, a model of 12
        train.main((config, mc), tdm_source=bad)
