"""transforms.mcs_aug (transforms.py:202-291: tf_cond, is_invertible, stab, mcs_aug) in its literal form, torch float64 on the CPU: the
[B,T,F,C,C] outer products, the condition number from the singular values, inv and det of the scaled matrix, all six stab steps.  The checker of
seld_aug_mcs; shared by tests/test_mcs_cpu.py, tests/test_mcs_gpu.py and tools/bench_mcs.py."""
import math

import torch

DD = (1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1)
EPS_INV = 1e6           # is_invertible: cond < 1 / epsilon, epsilon = 1e-6
MARGIN = 1.25           # no finite cond of a case may lie within this factor of EPS_INV

# name -> ((B, T, F, C), iteration, seed); the first case draws torch.rand (transforms_test.py:97-102), the others torch.randn
CASES = {
    "reference_test": ((3, 7, 4, 2), 2, 1),
    "single_frame": ((1, 1, 2, 3), 1, 6),
    "rank_deficient": ((2, 3, 4, 4), 2, 15),
    "past_a_wave": ((2, 65, 3, 7), 3, 2),
    "past_256_widest": ((1, 257, 2, 10), 2, 3),
    "one_channel": ((2, 130, 2, 1), 2, 5),
    "masked": ((1, 300, 5, 7), 2, 7),
    "full_clip": ((1, 3000, 1, 7), 1, 8),
}


def case_input(name):
    shape, iteration, seed = CASES[name]
    torch.manual_seed(seed)
    x = (torch.rand(shape) if name == "reference_test" else torch.randn(shape)).float()
    if name == "masked":
        x[:, :, 1, :] = 0                      # an all-zero column
        x[:, :, 2, :] = x[:, :1, 2, :]         # a constant column
        x[:, 100:124] = 0                      # a time mask
    return x, iteration


def safe_div(x, y, eps=1e-8):
    return x / torch.clamp(y, min=eps)


def cond_svd(m):
    """tf_cond: sigma_max / sigma_min; a NaN ratio from NaN-free input counts as infinite"""
    s = torch.linalg.svdvals(m)
    r = s[..., 0] / s[..., -1]
    x_nan = torch.isnan(m).any(-1).any(-1)
    return torch.where(x_nan, r, torch.where(torch.isnan(r), torch.full_like(r, math.inf), r))


def cond_eigh(m):
    """the same number from a symmetric eigen-solve (|lambda|max / |lambda|min): what the kernel computes"""
    e = torch.linalg.eigvalsh(m).abs()
    r = e.max(-1).values / e.min(-1).values
    return torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)


def is_invertible(m, cond=cond_svd):
    c = cond(m)
    return torch.isfinite(c) & (c < EPS_INV), c


def stab(m, cond=cond_svd, early_stop=False):
    """-> (matrix, additions per matrix int32, [cond evaluated at each step]).  early_stop: a matrix that has tested invertible is not tested
    again (it no longer changes); the literal form tests all six times."""
    eye = torch.eye(m.shape[-1], dtype=m.dtype)
    adds = torch.zeros(m.shape[:-2], dtype=torch.int32)
    done = torch.zeros(m.shape[:-2], dtype=torch.bool)
    conds = []
    for i in range(6):
        ok, c = is_invertible(m, cond)
        conds.append(torch.where(done, torch.full_like(c, math.nan), c) if early_stop else c)
        bad = ~ok & ~done if early_stop else ~ok
        if early_stop:
            done = done | ok
        m = m + (bad.to(m.dtype) * DD[i])[..., None, None] * eye
        adds = adds + bad.to(torch.int32)
    return m, adds, conds


def mcs(x, iteration, theta=1e-6, trace=None):
    """x [B,T,F,C] float32 -> dict(out float32 [B,T,F,C], lam float64 [B,T,F], stab_adds int32 [B,F,2,iteration+1], conds: every cond
    evaluated, one flat float64 tensor).  trace: a list that receives, per stab call, dict(R, A, inv, phi (the phi the round divides by), x)."""
    B, T, F, C = x.shape
    x32 = x
    x = x.double()
    xt = x.permute(0, 2, 3, 1)                                             # [B,F,C,T]
    r_y = xt @ x.permute(0, 2, 1, 3) / T                                   # [B,F,C,C]
    r_n = torch.eye(C, dtype=x.dtype).expand(B, F, C, C).clone()
    yyh = x[..., :, None] * x[..., None, :]                                # [B,T,F,C,C]
    adds, conds = [], []

    def stabbed(r):
        a, n, c = stab(r)
        adds.append(n)
        conds.extend(c)
        return a, torch.linalg.inv(a)

    def phi_of(inv):
        return torch.diagonal(yyh @ inv[:, None], dim1=-2, dim2=-1).sum(-1) / C      # trace(yyh inv) / C   [B,T,F]

    a_y, i_y = stabbed(r_y)
    a_n, i_n = stabbed(r_n)
    phi_y, phi_n = phi_of(i_y), phi_of(i_n)
    lam_n = None
    for _ in range(iteration):
        a_y, i_y = stabbed(r_y)
        a_n, i_n = stabbed(r_n)
        if trace is not None:
            trace.append(dict(x=x, A=(a_y, a_n), inv=(i_y, i_n), phi=(phi_y, phi_n)))
        p = []
        for a, inv, phi in ((a_n, i_n, phi_n), (a_y, i_y, phi_y)):
            k = x[..., None, :] @ safe_div(inv[:, None], phi[..., None, None])
            k = (k @ x[..., None]).squeeze(-1).squeeze(-1)
            det = torch.linalg.det(phi[..., None, None] * a[:, None]) * math.pi
            p.append(safe_div(torch.exp(-k), det) + theta)
        p_n, p_y = p
        lam_n, lam_y = safe_div(p_n, p_n + p_y), safe_div(p_y, p_n + p_y)
        phi_n, phi_y = phi_of(i_n), phi_of(i_y)
        acc_y = safe_div(lam_y, phi_y)[..., None, None] * yyh
        acc_n = safe_div(lam_n, phi_n)[..., None, None] * yyh
        r_y = safe_div(acc_y.sum(1), lam_y.sum(1)[..., None, None])
        r_n = safe_div(acc_n.sum(1), lam_n.sum(1)[..., None, None])
    out = x32 * lam_n[..., None].float()
    # adds: [y0, n0, y1, n1, ...] each [B,F] -> [B,F,2,iteration+1]
    sa = torch.stack([torch.stack(adds[0::2], -1), torch.stack(adds[1::2], -1)], 2)
    return dict(out=out, lam=lam_n, stab_adds=sa.contiguous(), conds=torch.cat([c.reshape(-1) for c in conds]))
