"""Times time-domain mixing on the device (recorded with no target: nobody had measured any of this).

At the real shape, a chunk of 32 clips of [4, 1 440 000] samples (60 s at 24 kHz, 600 label frames of 2400 samples, 12 classes), with K = 3 and
K = 5 insertions per clip of 5 .. 49 label frames drawn as data_loader.draw_tdm draws them from a bank of 12 classes:
  labels        seld_aug_tdm_labels on fresh labels (restored before every call, outside the timed window)
  mix in place  seld_aug_tdm_mix, x_out == x_in: only the covered frames move.  Beside it the bytes they move, counted from the plan (per covered
                frame one read and one write of the clip's C x spf samples and one read of the bank's per covering insertion), and that over
                the time as a fraction of 6.3 TB/s (what HBM3E sustains of its 8 TB/s peak)
  mix out of place   into a chunk buffer, as get_tdm_dataset does: every frame is read and written once
  features      FeatureExtractor.batch on the mixed chunk (n_fft = win_length = 1024, hop 480, 64 mels, foa): the stage behind the mix
HIP events around --reps calls after --warmup calls.  Then one whole regeneration, train.get_tdm_dataset over --clips clips (draws, labels, mix,
features, float64 statistics over the clip axis, normalisation, windows), host clock around a call that ends in a synchronise, the second of two
calls, on the schedule's first setting (1 insertion of 0.5 - 1 s) and its last (3 of 0.5 - 3 s).

python tools/bench_tdm.py [--reps 20] [--warmup 3] [--clips 400]  -> one JSON line, also written to profiles/tdm.json
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

HBM_BYTES_PER_S = 6.3e12
B, CH, T, SPF, NC = 32, 4, 600, 2400, 12


def timed(call, reps, warmup, before=None):
    for _ in range(warmup):
        if before:
            before()
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        if before:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms = np.array(ms)
    return {"ms_median": float(np.median(ms)), "p10": float(np.percentile(ms, 10)), "p90": float(np.percentile(ms, 90))}


def device_bank(dl, rows, gen):
    """a bank of random waveforms and one-class label tracks, made on the device (the host never holds the waves)"""
    tdm_x = [0.1 * torch.randn((CH, int(r) * SPF), generator=gen, device="cuda") for r in rows]
    tdm_y = []
    for k, r in enumerate(rows):
        lab = np.zeros((int(r), 4, NC), np.float32)
        lab[:, 0, k] = 1
        lab[:, 1, k] = 1
        tdm_y.append(lab.reshape(int(r), 4 * NC))
    return dl.TdmBank(tdm_x, tdm_y, 24000, 0.1)


def labels(n, rng):
    """[n, T, 4*NC]: a few events per clip, as a DCASE clip has"""
    y = np.zeros((n, T, 4, NC), np.float32)
    for i in range(n):
        for _ in range(12):
            c, a, d = int(rng.integers(NC)), int(rng.integers(T - 60)), int(rng.integers(10, 60))
            y[i, a:a + d, 0, c] = 1
            y[i, a:a + d, 1, c] = 1
    return y.reshape(n, T, 4 * NC)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--clips", type=int, default=400)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tdm.json"))
    a = ap.parse_args()
    from seld_amd import _lib, data_loader as dl, train
    from seld_amd.feature_extractor import FeatureExtractor
    if not torch.cuda.is_available():
        raise SystemExit("bench_tdm.py needs a HIP device: a time taken elsewhere says nothing")
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    rng = np.random.default_rng(0)
    gen = torch.Generator(device="cuda").manual_seed(0)
    rows = rng.integers(100, 600, NC)
    bank = device_bank(dl, rows, gen)
    x = 0.1 * torch.randn((B, CH, T * SPF), generator=gen, device="cuda")
    out = torch.empty_like(x)
    y0 = torch.as_tensor(labels(B, rng)).cuda()
    y = y0.clone()
    fe = FeatureExtractor(24000, "foa", 64, n_fft=1024, win_length=1024, hop_length=480)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "hbm_bytes_per_s": HBM_BYTES_PER_S,
           "chunk": [B, CH, T * SPF], "spf": SPF, "bank_rows": [int(r) for r in rows], "K": {}}
    for K in (3, 5):
        plan = dl.draw_tdm(rng, B, T, rows, K, 5, 50)
        ld = int(plan[..., 1].max())
        d_plan = torch.as_tensor(plan).cuda()
        valid = torch.empty((B, K, ld), device="cuda")

        def call_labels():
            rc = lib.seld_aug_tdm_labels(p(y), B, T, 4 * NC, p(bank.bank_y), p(bank.d_row0), p(bank.d_rows), NC, p(d_plan), K, 2, p(valid), ld, stream)
            assert rc == 0, rc

        def call_mix(dst):
            rc = lib.seld_aug_tdm_mix(p(x), p(dst), B, CH, T * SPF, T, SPF, p(bank.bank_x), p(bank.d_s0), NC, p(d_plan), K, p(valid), ld, stream)
            assert rc == 0, rc
        row = {"labels": timed(call_labels, a.reps, a.warmup, before=lambda: y.copy_(y0))}
        y.copy_(y0)
        call_labels()                                   # valid of the fresh labels: what the mix is timed with
        torch.cuda.synchronize()
        cover = np.zeros((B, T), np.int64)              # insertions that cover each (clip, label frame)
        for b in range(B):
            for cls, st, off, td in plan[b]:
                cover[b, off:off + st] += 1
        frame_bytes = CH * SPF * 4
        moved = int((cover > 0).sum() * 2 * frame_bytes + cover.sum() * frame_bytes)
        row["valid_fraction"] = float(valid.cpu().numpy().sum() / max(1, plan[..., 1].sum()))
        row["covered_frames"] = int((cover > 0).sum())
        row["frames"] = B * T
        m = timed(lambda: call_mix(x), a.reps, a.warmup)
        m.update(bytes_moved=moved, bytes_per_s=moved / (m["ms_median"] * 1e-3), hbm_fraction=moved / (m["ms_median"] * 1e-3) / HBM_BYTES_PER_S)
        row["mix_in_place"] = m
        x.normal_(0, 0.1, generator=gen)                # the in-place calls accumulated into x
        moved_out = int(2 * x.numel() * 4 + cover.sum() * frame_bytes)
        m = timed(lambda: call_mix(out), a.reps, a.warmup)
        m.update(bytes_moved=moved_out, bytes_per_s=moved_out / (m["ms_median"] * 1e-3), hbm_fraction=moved_out / (m["ms_median"] * 1e-3) / HBM_BYTES_PER_S)
        row["mix_out_of_place"] = m
        f = timed(lambda: fe.batch(out), a.reps, a.warmup)
        f["clips_per_s"] = B / (f["ms_median"] * 1e-3)
        row["features"] = f
        row["finite"] = bool(torch.isfinite(out).all())
        res["K"][str(K)] = row
    del x, out
    # one whole regeneration
    n = a.clips
    src_x = torch.empty((n, CH, T * SPF), device="cuda").normal_(0, 0.1, generator=gen)
    source = train.TdmSource(src_x, torch.as_tensor(labels(n, rng)).cuda(), bank)
    cfg = argparse.Namespace(batch=256, loop_time=5, use_tfm=False, use_acs=False)
    res["regeneration"] = {"clips": n, "source_bytes": int(src_x.numel() * 4)}
    for name, kw in (("schedule_first", dict(max_overlap_num=1, min_overlap_sec=0.5, max_overlap_sec=1)),
                     ("schedule_last", dict(max_overlap_num=3, min_overlap_sec=0.5, max_overlap_sec=3))):
        wall = []
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ds = train.get_tdm_dataset(cfg, max_overlap_per_frame=2, source=source, rng=rng, **kw)
            torch.cuda.synchronize()
            wall.append(time.perf_counter() - t0)
        res["regeneration"][name] = {"wall_s_first_call": wall[0], "wall_s": wall[1], "clips_per_s": n / wall[1], "windows": int(ds.x.shape[0]),
                                     "finite": bool(torch.isfinite(ds.x).all())}
        del ds
    line = json.dumps(res)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
