"""What the cases of tests/gemm_cases.py promise, checked without a GPU, so that a failure of tests/test_gemm_family_gpu.py means the kernel:
the tables cover what they claim, every reference is finite, a plain float32 numpy evaluation of every case stays within half of the bar the GPU
test applies to it, what is zero by construction is exactly zero in the reference, every listed refusal follows from the launcher's conditions,
and the four-product form's own arithmetic stays under the figure its bar is built from."""
import numpy as np
import pytest

import gemm_cases as G
from gemm_cases import f64


def half_bar(name, got32, ref, mag, bar):
    assert np.isfinite(ref).all() and np.isfinite(mag).all(), name
    G.report(f"fp32 numpy: {name}", G.mag_err(got32, ref, mag), bar / 2)


# ---------------------------------------------------------------- tables
def test_f32_cross_keeps_every_value_with_both_transb():
    for tb in (0, 1):
        cs = [c for c in G.F32_CROSS if c.transb == tb]
        assert {c.M for c in cs} == set(G.F32_MS) and {c.N for c in cs} == set(G.F32_NS) and {c.K for c in cs} == set(G.F32_KS)
        assert {c.ld for c in cs} == set(G.F32_LDS)
        assert any(c.K == 32 and c.ld == "pad4" for c in cs) and any(c.K == 32 and c.ld == "tight" for c in cs)      # the vector loads, padded and not
    assert len(set(G.F32_CASES)) == len(G.F32_CASES)
    # B's float4 loads under a padded ldb, transb = 0: N % 4 == 0, which no N of the cross is
    assert all(n % 4 for n in G.F32_NS) and any(c.transb == 0 and c.N % 4 == 0 and c.ld == "pad4" and G.f32_lds(c)[1] % 4 == 0 for c in G.F32_CASES)
    for n0, n1 in G.F32_HEADS:
        assert n0 + n1 >= 2
    assert [n0 % 64 == 0 for n0, _ in G.F32_HEADS] == [False, False, False, True] and G.F32_HEADS[2][0] > 64


def test_tn_cases_take_the_splits_they_name():
    for c in G.TN_CASES:
        assert G.tn_splits(c.M, c.max_splits, c.chunk) == c.nslab, c
        if c.shift:
            assert c.M % c.S == 0
    assert {c.M for c in G.TN_CASES} >= {1, 31, 32, 33, 160, 161, 321}
    assert {c.K1 for c in G.TN_CASES} == {c.N for c in G.TN_CASES} == {1, 63, 64, 65, 129}
    assert {c.M for c in G.TN_CASES if c.chunk == 64} >= {65, 129, 321}
    assert {c.max_splits for c in G.TN_CASES} == {0, 1, 3}
    # a last split of a single row; a split boundary (rows per split, from the rule) on a sequence boundary under S = 5 and inside a sequence under S = 7
    rps = lambda c: -(-(-(-c.M // min((c.M + 159) // 160, c.max_splits or 128))) // c.chunk) * c.chunk
    assert any(c.M % rps(c) == 1 and c.nslab > 1 for c in G.TN_CASES)
    assert any(c.S == 5 and c.nslab > 1 and rps(c) % 5 == 0 for c in G.TN_CASES) and any(c.S == 7 and c.nslab > 1 and rps(c) % 7 for c in G.TN_CASES)
    for K1, N, M in G.TNSB_TILES:
        assert G.tn_tile_splits(M, K1, N, K1 * N) == 1 and G.tn_tile_splits(M, K1, N, 8 * K1 * N) == (M + 127) // 128 > 1


def test_sb_tables():
    assert set(G.SB_UNROLLED16.values()) == {4, 8, 12, 16, 24, 36}
    for (K, mode), ng in G.SB_UNROLLED16.items():
        assert K // 32 * (2 if mode == 2 else 1) == ng and (K, mode) in G.SB_KS
    assert {(K, m) for K, m in G.SB_KS} - set(G.SB_UNROLLED16) == {(32, 0), (96, 0), (160, 0)}
    for C, (B, H, W) in G.SB_CONV:
        assert C & (C - 1) == 0 and C >= 32 and B * H * W < 128
    # every pixel of the three images is on a border, and with M < 128 a batch boundary falls inside the one tile
    for B, H, W in G.CONV_IMAGES:
        assert (H <= 2 or W <= 2) and B * H * W < 128


# ---------------------------------------------------------------- refusals
def test_refusals_follow_from_the_launchers():
    for name, kw in G.F32_REFUSALS:
        assert G.gemm_go_refuses(**kw), name
        base = dict(kw, bias=False, act=0, accumulate=0, addg=False, mode=0, M=max(kw["M"], 1))
        assert not G.gemm_go_refuses(**base), name
    for name, kw in G.SB_REFUSALS:
        assert G.gemm_sb_refuses(**kw), name
    assert not G.gemm_sb_refuses(M=33, N=128, K=96, mode=2) and not G.gemm_sb_refuses(M=33, N=128, K=96, stat=True)
    assert not G.gemm_sb_refuses(M=12, N=128, K=288, conv_C=32, H=3, W=2) and not G.gemm_sb_refuses(M=33, N=128, K=96, ldc=132, addg=True)
    assert G.heads_refuses(5, 30, 35) and not G.heads_refuses(5, 14, 50)
    assert G.heads_refuses(576, 1, 2, prep=True) and not G.heads_refuses(575, 1, 2, prep=True) and not G.heads_refuses(576, 1, 2)
    for K, Hd, n0, n1 in G.HEADS_CASES:
        assert not G.heads_refuses(K, n0, n1, prep=True)


# ---------------------------------------------------------------- fp32 numpy within half of each bar
@pytest.mark.parametrize("c", G.F32_CASES, ids=G.f32_id)
def test_f32_cases_fp32_numpy(c):
    A, B, bias, prev, A1, B1, bias1 = G.f32_inputs(c.M, c.N, c.K, c.transb)
    ref, mag = G.product(A, B, c.transb, bias)
    half_bar(G.f32_id(c), G.product32(A, B, c.transb, bias), ref, mag, G.BAR6)


def test_f32_epilogues_fp32_numpy():
    for M, N, K, _ in G.F32_EPI_SHAPES:
        for tb in (0, 1):
            A, B, bias, prev, A1, B1, bias1 = G.f32_inputs(M, N, K, tb)
            A = A * G.EPI_SCALE
            for act in range(4):
                for acc in (None, prev):
                    ref, mag = G.product(A, B, tb, bias, act, acc)
                    half_bar(f"{M, N, K} tb{tb} act{act} acc{acc is not None}", G.product32(A, B, tb, bias, act, acc), ref, mag, G.BAR6)
    for K in (32, 64):
        A, B, bias, prev, A1, B1, bias1 = G.f32_inputs(65, 63, K, 0)
        ref, mag = G.product(A, B, 0, bias, 0, prev, A1, B1)
        half_bar(f"mode 2 K{K}", G.product32(A, B, 0, bias, 0, prev, A1, B1), ref, mag, G.BAR6)


@pytest.mark.parametrize("K,mode", G.SB_KS)
def test_sb_cases_fp32_numpy(K, mode):
    for tb in (0, 1):
        A0, A1, B0, B1, b0, b1, prev, addg = G.sb_inputs(129, 128, K, tb)
        kw = dict(A1=A1, B1=B1) if mode == 2 else {}
        ref, mag = G.product(A0, B0, tb, b0, **kw)
        half_bar(f"sb K{K} mode{mode} tb{tb}", G.product32(A0, B0, tb, b0, **kw), ref, mag, G.BAR6)


def test_sb_rows_and_conv_fp32_numpy():
    for M in G.SB_MS:
        A0, A1, B0, B1, b0, b1, prev, addg = G.sb_inputs(M, 128, 128, 0)
        ref, mag = G.product(A0, B0, 0, b0)
        half_bar(f"sb M{M}", G.product32(A0, B0, 0, b0), ref, mag, G.BAR6)
    for C, img in G.SB_CONV:
        x, w, dz = G.conv_inputs(C, img)
        ref, mag = G.conv_fwd_ref(x, w)
        col = G.im2col3x3(x)
        half_bar(f"conv C{C} {img}", G.matmul32(col, w.reshape(9 * C, -1)), ref, mag, G.BAR6)
        # the im2col statement of the operation equals conv2d: the tap order the kernels assume
        np.testing.assert_allclose(f64(col) @ f64(w.reshape(9 * C, -1)), ref, rtol=0, atol=1e-12 * mag.max())
    for C, img in G.SB_CONV_BWD:
        x, w, dz = G.conv_inputs(C, img)
        dx, dw = G.conv_grads_ref(x, w, dz)
        np.testing.assert_allclose(f64(G.im2col3x3(dz)) @ f64(G.dgrad_matrix(w)), dx, rtol=0, atol=1e-12 * np.abs(dx).max())
        np.testing.assert_allclose(f64(G.im2col3x3(x)).T @ f64(dz.reshape(-1, dz.shape[3])), dw, rtol=0, atol=1e-12 * np.abs(dw).max())


@pytest.mark.parametrize("c", G.TN_CASES, ids=G.tn_id)
def test_tn_cases_fp32_numpy(c):
    A, B = G.tn_inputs(c.M, c.K1, c.N)
    ref, mag, cs, csmag = G.tn_ref(A, B, c.M, c.S, c.shift)
    As = G.shifted(A, c.M, c.S if c.S else c.M, c.shift)
    half_bar(G.tn_id(c), G.matmul32(As.T, B), ref, mag, G.BAR6)
    half_bar(G.tn_id(c) + " colsum", B.sum(0, dtype=np.float32), cs, csmag, G.BAR6)
    if c.S == 1:
        assert not ref.any() and not mag.any()      # zero by construction: every shifted row is masked


def test_tnsb_cases_fp32_numpy():
    for M in G.TNSB_MS:
        for N in (128, 256):
            for j, (shift, _) in enumerate(G.TNSB_JOBS):
                A, B = G.tnsb_inputs(M, N, j)
                ref, mag, cs, csmag = G.tn_ref(A, B, M, G.TNSB_S, shift)
                half_bar(f"tn_sb M{M} N{N} job{j}", G.matmul32(G.shifted(A, M, G.TNSB_S, shift).T, B), ref, mag, G.BAR6)
                half_bar(f"tn_sb M{M} N{N} job{j} colsum", B.sum(0, dtype=np.float32), cs, csmag, G.BAR6)
    for K1, N, M in G.TNSB_TILES:
        A, B = G.tn_inputs(M, K1, N)
        ref, mag, _, _ = G.tn_ref(A, B, M)
        half_bar(f"tn_sb tiles {K1, N, M}", G.matmul32(A.T, B), ref, mag, G.BAR6)


def test_gates_all_off_is_exactly_zero():
    g, on = G.gates(33, 132, all_off=True)
    assert not g.any() and not on.any()
    g, on = G.gates(129, 132)
    assert 0.3 < on.mean() < 0.7 and g.size == (129 * 132 + 3) // 4
    # a wrong stride or a bit taken from the lane picks other bits
    e = np.arange(129 * 132)
    assert (on.reshape(-1) != ((g[(e // 132 * 128 + e % 132) >> 2] >> (e & 3)) & 1)).mean() > 0.2


def test_heads_and_reductions_fp32_numpy():
    for case in G.HEADS_CASES:
        heads, F, cs = G.heads_inputs(*case)
        ref, mag = G.heads_weff_ref(heads)
        got = np.concatenate([np.vstack([G.matmul32(w1, w2), G.matmul32(b1[None], w2) + b2]) for w1, b1, w2, b2 in heads], axis=1)
        half_bar(f"weff {case}", got, ref, mag, G.BAR6)
        c0 = 0
        for (w1, b1, w2, b2), grads in zip(heads, G.heads_grad_ref(heads, F, cs)):
            n = w2.shape[1]
            Fh, ch = F[:, c0:c0 + n], cs[c0:c0 + n]
            got32 = (G.matmul32(Fh, w2.T), G.matmul32(ch[None], w2.T)[0], G.matmul32(w1.T, Fh) + np.outer(b1, ch), ch)
            for label, g32, (r, m) in zip(("dW1", "db1", "dW2", "db2"), got32, grads):
                half_bar(f"heads_grad {case} {label}", g32, r, m, G.BAR6)
            c0 += n
    for ns in G.RED_NSLABS + G.RED_2STAGE:
        s = G.slabs(ns, 104)
        half_bar(f"slabs {ns}", s.sum(0, dtype=np.float32), f64(s).sum(0), np.abs(f64(s)).sum(0), G.BAR6)


def test_f32_heads_and_stat_part_fp32_numpy():
    """mode 4 (each head's columns with its own activation) and the BatchNorm partials: fp32 sums of the fp32 product's rows against fp64 sums of the
    same rows, at the row blocks of either kernel family"""
    for n0, n1 in G.F32_HEADS:
        A, B, bias, prev, A1, B1, bias1 = G.f32_inputs(65, n0 + n1, 33, 0)
        A = A * G.EPI_SCALE
        for act0, act1 in ((1, 2), (2, 1), (0, 1)):
            for sl, act in ((slice(0, n0), act0), (slice(n0, None), act1)):
                ref, mag = G.product(A, B[:, sl], 0, bias[sl], act)
                half_bar(f"mode 4 n{n0}+{n1} act{act}", G.product32(A, B[:, sl], 0, bias[sl], act), ref, mag, G.BAR6)

    def partials32(Cm, rb):
        out = []
        for ch in range(-(-Cm.shape[1] // 64)):
            for by in range(-(-Cm.shape[0] // rb)):
                blk = Cm[by * rb:(by + 1) * rb, ch * 64:(ch + 1) * 64]
                row = np.zeros(128, np.float32)
                row[:blk.shape[1]], row[64:64 + blk.shape[1]] = blk.sum(0, dtype=np.float32), (blk * blk).sum(0, dtype=np.float32)
                out.append(row)
        return np.concatenate(out)[None]
    M, N, K = G.F32_STAT
    for N_ in (N, 96):
        A, B = G.f32_inputs(M, N_, K, 0)[:2]
        Cm = G.product32(A, B)
        half_bar(f"stat_part f32 N{N_}", partials32(Cm, 64), *G.stat_ref(Cm, 64), G.BAR6)
    for M in (129, 33):
        i = G.sb_inputs(M, 128, 128, 0)
        Cm = G.product32(i[0], i[2])
        half_bar(f"stat_part sb M{M}", partials32(Cm, 128), *G.stat_ref(Cm, 128), G.BAR6)


# ---------------------------------------------------------------- the four-product form
def test_four_product_emulation():
    """two planes per operand with the rounded mid, the four retained products, fp64 accumulation: the error of the FORM, on the GPU cases' own inputs"""
    worst = 0.0
    for name, A, B in G.four_cases():
        ref, mag = f64(A) @ f64(B), np.abs(f64(A)) @ np.abs(f64(B))
        e = G.mag_err(G.two_planes_rounded(A) @ G.two_planes_rounded(B), ref, mag)
        print(f"[four] {name:40s} emulation err / (|A| |B|) = {e:.3e}")
        worst = max(worst, e)
    print(f"[four] largest = {worst:.3e}; FOUR_EMUL = {G.FOUR_EMUL:.3e}; BAR4 = {G.BAR4:.3e}")
    assert worst <= G.FOUR_EMUL and G.FOUR_EMUL <= 1.25 * worst and G.BAR4 < 1e-4


def test_plane_helpers():
    x = G.binade(np.random.default_rng(0), (4096,))
    two = G.two_planes_rounded(x)
    assert np.abs(two - f64(x)).max() <= 2.0 ** -16 * np.abs(x).max() and (np.abs(two - f64(x)) <= 2.0 ** -16 * np.abs(f64(x))).all()
    import torch
    np.testing.assert_array_equal(G.bf16_rne(x), torch.as_tensor(x).bfloat16().double().numpy())
