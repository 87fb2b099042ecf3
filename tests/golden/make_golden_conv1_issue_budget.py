"""Records tests/golden/conv1_issue_budget/{kernel,train}.npz: what the first block's z-free forward (csrc/conv_pool_sb.hip) and two seldnet train
steps computed with the library of the commit BEFORE the epilogue of that file was re-counted in issue slots (scalar BatchNorm sums, v_max3_f32,
branch-free position search).  tests/test_conv1_issue_budget_gpu.py holds every later build to these bits, so the fixtures must not come
from the code under test: build the parent commit's library somewhere else and name it in SELD_HIP_LIB.  On an MI355X, from the repository root:

    SELD_HIP_LIB=/path/to/parent/libseld_hip.so python tests/golden/make_golden_conv1_issue_budget.py [output directory]

Inputs, weights and gamma are regenerated from fixed seeds by the test through the functions below.  kernel.npz: per case zext (one array: the
recorder asserts that the three forms agree), amax of the two forms that write it, and the 128 statistics sums.  train.npz: outputs, losses and
BatchNorm state in full; of the gradients and weights (0.5 M floats each, five arrays: 10 MB) a strided sample and the SHA-256 of their bytes."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FIXTURE_DIR = os.path.join(ROOT, "tests", "golden", "conv1_issue_budget")
# (B, H, Cin): tiles = B * ceil(H / 10).  Cin = 10 runs the 4-wave kernel, which shares the epilogue macros
CASES = [(1, 10, 7),     # one tile, and one wave group without work
         (1, 15, 7),     # a tile with a dead pooling row
         (3, 25, 7),     # odd virtual grid, tile streams of unequal length inside a block
         (2, 40, 7),
         (1, 10, 10)]
# (amax, statistics): training, positions without statistics, inference
FORMS = [(True, True), (True, False), (False, False)]
TRAIN_B, TRAIN_T = 2, 50
SAMPLE = 4096


def case_name(B, H, Cin):
    return f"b{B}_h{H}_c{Cin}"


def plant_ties(x):
    """Exact ties inside pooling windows (5 rows x 4 bins): the 3 x 3 neighbourhood of one pixel copied onto another pixel of the same window whose
    neighbourhood does not overlap it (rows 1 and 4 of the window), so both pixels get the same bits in every output channel.  Three kinds by
    window: same column; the later row in a LATER column; the later row in an EARLIER column (scan order is column-major: that one must win).
    Returns the list of (b, pooled row, window column, (row, col) of the source, (row, col) of the copy)."""
    B, H = x.shape[:2]
    planted = []
    for b in range(B):
        for k in range(H // 5 - 1):          # rows 5 k .. 5 k + 5 exist
            for m in range(1 + (k + b) % 2, 15, 2):
                kind = (k + m + b) % 3
                cs, cd = ((1, 1), (0, 2), (2, 0))[kind]
                ts, td = 5 * k + 1, 5 * k + 4
                x[b, td - 1:td + 2, 4 * m + cd - 1:4 * m + cd + 2] = x[b, ts - 1:ts + 2, 4 * m + cs - 1:4 * m + cs + 2]
                planted.append((b, k, m, (1, cs), (4, cd)))
    return planted


def kernel_inputs(B, H, Cin):
    """x [B, H, 64, Cin] with planted ties, w [3, 3, Cin, 64], bias [64], gamma [64] (both signs, 8 or more negative, one zero), and the ties"""
    rng = np.random.default_rng(20240 + 100 * B + H + Cin)
    x = rng.standard_normal((B, H, 64, Cin)).astype(np.float32)
    planted = plant_ties(x)
    w = (rng.standard_normal((3, 3, Cin, 64)) / np.sqrt(9 * Cin)).astype(np.float32)
    bias = rng.standard_normal(64).astype(np.float32)
    gamma = (rng.uniform(0.5, 1.5, 64) * np.where(rng.random(64) < 0.3, -1, 1)).astype(np.float32)
    gamma[1:32:4] = -np.abs(gamma[1:32:4])     # eight negative channels whatever the draw, in both channel halves of a lane
    gamma[34:64:8] = -np.abs(gamma[34:64:8])
    gamma[5] = 0.0
    assert (gamma < 0).sum() >= 8 and (gamma > 0).sum() >= 8
    return x, w, bias, gamma, planted


def run_kernel(lib, dev_args, B, H, Cin, with_amax, with_stats):
    """seld_k_conv_first_fwd_pool with z == NULL -> zext, amax, statistics as numpy arrays (NaN / 255 where the kernel wrote nothing)"""
    import torch
    from helpers import ptr
    ze = torch.full((B, H // 5, 16, 64), float("nan"), device="cuda")
    am = torch.full((B, H // 5, 16, 64), 255, device="cuda", dtype=torch.uint8)
    st = torch.full((128,), float("nan"), device="cuda")
    xd, wd, bd, gd = dev_args
    rc = lib.seld_k_conv_first_fwd_pool(ptr(xd), ptr(wd), ptr(bd), ptr(gd), None, ptr(ze), ptr(am) if with_amax else None,
                                        ptr(st) if with_stats else None, B, H, Cin)
    torch.cuda.synchronize()
    assert rc == 0, rc
    return ze.cpu().numpy(), am.cpu().numpy(), st.cpu().numpy()


def train_items(config):
    """Two train steps of seldnet on [2, 50, 64, 7]: name -> array (outputs, losses and gradients of both steps, final weights and BatchNorm state)"""
    from oracle import seldnet_oracle as O
    from seld_amd import losses, models, train
    spec = O.Spec.from_config(config)
    w, st = O.random_weights(spec, 0)
    x, ys, yd = O.synthetic_batch(TRAIN_B, TRAIN_T, seed=1234)
    model = models.seldnet((TRAIN_B, TRAIN_T, 64, 7), config)
    model.set_weights(w, st)
    got = {}
    opt_ = train.Adam(1e-3)
    for i in range(2):
        y_p, sl, dl = train.trainstep(model, x, (ys, yd), losses.BinaryCrossentropy(), losses.MMSE, (1.0, 1000.0), opt_)
        got[f"sed{i}"], got[f"doa{i}"] = y_p[0].cpu().numpy().copy(), y_p[1].cpu().numpy().copy()
        got[f"sloss{i}"], got[f"dloss{i}"] = sl.cpu().numpy().copy(), dl.cpu().numpy().copy()
        got[f"grad{i}"] = np.array(model.get_grads(), copy=True)
    weights, state = model.get_weights()
    got["weights"], got["state"] = np.array(weights, copy=True), np.array(state, copy=True)
    model.close()
    return got


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8).copy()


def fixture_form(items):
    """What train.npz keeps of train_items(): small arrays whole, large ones as a strided sample and the SHA-256 of their bytes"""
    out = {}
    for k, v in items.items():
        v = np.ascontiguousarray(v)
        if v.size <= SAMPLE:
            out[k] = v
        else:
            out[k + ".sample"] = v.reshape(-1)[np.linspace(0, v.size - 1, SAMPLE).astype(np.int64)]
            out[k + ".sha256"] = digest(v)
            out[k + ".shape"] = np.array(v.shape, np.int64)
    return out


def main(out_dir):
    import torch
    from helpers import dev
    from seld_amd import _lib
    from __graft_entry__ import SELDNET_CONFIG
    assert os.environ.get("SELD_HIP_LIB"), "name the PARENT commit's library in SELD_HIP_LIB: the fixtures must not come from the code under test"
    assert torch.cuda.is_available()
    lib = _lib.load()
    os.makedirs(out_dir, exist_ok=True)
    out = {}
    for B, H, Cin in CASES:
        x, w, bias, gamma, planted = kernel_inputs(B, H, Cin)
        args = tuple(dev(a) for a in (x, w, bias, gamma))
        ze, am, st = run_kernel(lib, args, B, H, Cin, True, True)
        ze1, am1, _ = run_kernel(lib, args, B, H, Cin, True, False)
        ze2, am2, _ = run_kernel(lib, args, B, H, Cin, False, False)
        assert np.isfinite(ze).all() and np.isfinite(st).all() and am.max() < 20 and (am2 == 255).all()
        assert np.array_equal(ze, ze1) and np.array_equal(ze, ze2), "the three forms disagree on zext"
        # how many planted ties ARE the window extreme, i.e. decide a position
        won = 0
        for b, k, m, (rs, cs), (rd, cd) in planted:
            a = am[b, k, m]
            first, second = ((rs, cs), (rd, cd)) if (cs, rs) < (cd, rd) else ((rd, cd), (rs, cs))
            assert not (a == second[0] * 4 + second[1]).any(), "a tie went to the later pixel in scan order"
            won += int((a == first[0] * 4 + first[1]).sum())
        n = case_name(B, H, Cin)
        print(f"{n}: {len(planted)} planted ties, the earlier pixel is the extreme of {won} (window, channel) pairs; "
              f"{int((gamma < 0).sum())} negative channels", flush=True)
        out[n + ".zext"], out[n + ".amax"], out[n + ".amax_nostats"], out[n + ".stats"] = ze, am, am1, st
    path = os.path.join(out_dir, "kernel.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    items = train_items(SELDNET_CONFIG)
    assert all(np.isfinite(v).all() for v in items.values())
    path = os.path.join(out_dir, "train.npz")
    np.savez_compressed(path, **fixture_form(items))
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else FIXTURE_DIR)
