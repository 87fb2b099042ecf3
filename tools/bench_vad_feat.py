"""Times the voice-activity front end on a seeded corpus of a size a user would run — 512 utterances of 3 - 4 s at
16 kHz, n_fft 1024, 80 mel bands, log and min-max on — two ways in one call:

  fused      seld_vad_feat_extract (seld_amd/csrc/vad_feat.hip): the packed corpus in two launches
  composed   torch device operators per file: torch.stft(center=False, periodic Hann) magnitude, matmul with the dense mel matrix, clamp, log,
             min-max — the per-file arithmetic of vad_dataloader.py:86-97; the results are concatenated outside the timed window

A sample is HIP events on the stream around --reps passes over the corpus for the fused path (a pass is two launches) and one pass for the
composition (thousands of launches); the two paths alternate; median and p10 - p90 of --calls samples after
--warmup rounds.  Bytes come from shapes: the wav is read once (frames overlap by half, but the second read of a sample is an L2 hit of the
same workgroup's neighbour), `out` is written by the first kernel and read and written by the second.  The record holds utterances/s, GB/s,
the agreement of the two paths and `fused_wins`; there is no target: neither path had been measured before.  Prints one JSON line; --out
writes it to a file as well.  Needs a HIP device.

    python tools/bench_vad_feat.py [--files 512] [--calls 20] [--warmup 3] [--reps 10] [--out profiles/vad_feat.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

SR, N_FFT, N_MELS = 16000, 1024, 80


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
    ap.add_argument("--files", type=int, default=512)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_vad_feat needs a HIP device: nothing is measured without one")
    from seld_amd import _lib, vad_dataloader as L
    dev = torch.device("cuda", torch.cuda.current_device())
    rng = np.random.default_rng(0)
    lengths = rng.integers(3 * SR, 4 * SR + 1, a.files)
    t = np.arange(int(lengths.max())) / SR
    wavs = [(rng.uniform(0.05, 1.0) * (0.1 * rng.standard_normal(n) + 0.3 * np.sin(2 * np.pi * rng.uniform(100, 3000) * t[:n]))).astype(np.float32)
            for n in lengths]
    ss = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    fs = np.concatenate([[0], np.cumsum([L.n_frames(N_FFT, int(n)) for n in lengths])]).astype(np.int64)
    wav_d = torch.as_tensor(np.concatenate(wavs)).to(dev)
    ss_d, fs_d = torch.as_tensor(ss).to(dev), torch.as_tensor(fs).to(dev)
    out_d = torch.empty((int(fs[-1]), N_MELS), dtype=torch.float32, device=dev)
    fe = L._FrontEnd.get(SR, N_FFT, N_MELS, dev)
    lib = _lib.load()
    p = lambda x: C.c_void_p(x.data_ptr())

    def fused():
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(lib.seld_vad_feat_extract(fe.h, p(wav_d), p(ss_d), p(fs_d), a.files, int(ss[-1]), int(fs[-1]), 1, 1, p(out_d), st))

    mel = torch.as_tensor(L.get_mel_scale(N_FFT, N_MELS, SR)).to(dev)
    win = torch.hann_window(N_FFT, periodic=True, dtype=torch.float32, device=dev)
    views = [wav_d[int(ss[i]):int(ss[i + 1])] for i in range(a.files)]
    parts = [None] * a.files

    def composed():
        for i, x in enumerate(views):
            s = torch.stft(x, N_FFT, hop_length=N_FFT // 2, win_length=N_FFT, window=win, center=False, return_complex=True).abs().T @ mel
            s = torch.log(torch.minimum(torch.clamp_min(s, 1e-8), s.max()))
            lo, hi = s.min(), s.max()
            parts[i] = (s - lo) / (hi - lo)

    runs = {"fused": fused, "composed": composed}
    ts = {n: [] for n in runs}
    for r in range(a.calls + a.warmup):
        for n in runs:
            ms = timed(runs[n], a.reps if n == "fused" else 1)
            if r >= a.warmup:
                ts[n].append(ms)
    ref = torch.cat(parts)
    agreement = float((out_d - ref).abs().max() / ref.abs().max())
    # wav read once; out written (kernel 1), read and written (kernel 2)
    n_bytes = 4 * int(ss[-1]) + 3 * 4 * int(fs[-1]) * N_MELS
    med = {n: statistics.median(ts[n]) for n in runs}
    out = {"device": torch.cuda.get_device_name(0), "files": a.files, "seconds_of_audio": round(float(ss[-1]) / SR, 1), "sample_rate": SR,
           "n_fft": N_FFT, "n_mels": N_MELS, "total_frames": int(fs[-1]), "calls": a.calls, "warmup": a.warmup, "reps": a.reps,
           "fused_ms": stats(ts["fused"]), "composed_ms": stats(ts["composed"]), "fused_bytes": n_bytes,
           "fused_gb_per_s": round(n_bytes / (med["fused"] * 1e-3) / 1e9, 1),
           "fused_utterances_per_s": round(a.files / (med["fused"] * 1e-3), 1), "composed_utterances_per_s": round(a.files / (med["composed"] * 1e-3), 1),
           "composed_over_fused": round(med["composed"] / med["fused"], 2), "agreement_max_rel": agreement, "fused_wins": bool(med["fused"] < med["composed"])}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as o:
            o.write(line + "\n")


if __name__ == "__main__":
    main()
