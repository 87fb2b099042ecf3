"""fp64 restatement of the reference's configurable recurrent block, modules.RNN_block / RNN_stage (modules.py:64-83, 322-347), in Keras layout, as
explicit step loops with gradients by autograd: the LSTM and GRU cells, both directions of a Bidirectional, its four merges, the block and the stage,
and models.seldnet with SECOND = RNN_stage.  Checker only (torch on the CPU); the seeded input makers of tests/test_rnn_gpu.py's cases live here so
that tests/test_rnn_cpu.py can hold a plain fp32 evaluation of the same cases against fp64.

Keras LSTM(units, return_sequences=True) defaults: gate order i | f | c | o, ONE bias, activation tanh, recurrent_activation sigmoid:
  z = x kernel + bias + h U;  i = s(z_i)  f = s(z_f)  g = tanh(z_c)  o = s(z_o);  c' = f c + i g;  h' = o tanh(c')
The GRU cell (reset_after=True, gate order z | r | h, bias [2, 384]) is oracle.seldnet_oracle.gru_direction."""
import copy
import math

import numpy as np
import torch

import conformer_oracle as CF
import transformer_oracle as T
from oracle import modules_oracle as M
from oracle import seldnet_oracle as O

MERGES = ("mul", "concat", "ave", "sum")
U_ = 128


def f32(a):
    return np.asarray(a, np.float32)


# ---------------------------------------------------------------- the cells, from pre-computed input projections
def lstm_recurrence(gx, U, reverse: bool):
    """gx [B,S,4u] = x kernel + bias, U [u,4u] -> (h, c) [B,S,u]; reverse: Bidirectional's backward layer (t = S-1..0, written where consumed)"""
    B, S, _ = gx.shape
    u = U.shape[0]
    h, c = gx.new_zeros(B, u), gx.new_zeros(B, u)
    hs, cs = [None] * S, [None] * S
    for t in (range(S - 1, -1, -1) if reverse else range(S)):
        z = gx[:, t] + h @ U
        i, f, g, o = torch.sigmoid(z[:, :u]), torch.sigmoid(z[:, u:2 * u]), torch.tanh(z[:, 2 * u:3 * u]), torch.sigmoid(z[:, 3 * u:])
        c = f * c + i * g
        h = o * torch.tanh(c)
        hs[t], cs[t] = h, c
    return torch.stack(hs, 1), torch.stack(cs, 1)


def gru_recurrence(gx, U, brec, reverse: bool, probe=None, rec_mask=None, aux=None):
    """the step loop of oracle.seldnet_oracle.gru_direction from gx [B,S,3u] = x kernel + bias[0]; probe [B,S,3u] (zeros) is added to the recurrent-side
    pre-activation h U + bias[1], so that its gradient is the kernels' dgh.  rec_mask [B,u] (Keras recurrent_dropout; GRUCell.call, implementation
    2, as gru_direction states it): the previous state is multiplied by the mask before the recurrent product AND before the blend; the emitted h[t]
    is the unmasked state.  aux: a dict that receives what the kernels save for the backward pass, each [B,S,u]: z, r, hh and gh_h, the candidate
    gate's recurrent pre-activation h_prev U_h + brec_h"""
    B, S, _ = gx.shape
    u = U.shape[0]
    h = gx.new_zeros(B, u)
    hs = [None] * S
    kept = {k: [None] * S for k in ("z", "r", "hh", "gh_h")}
    for t in (range(S - 1, -1, -1) if reverse else range(S)):
        if rec_mask is not None:
            h = h * rec_mask
        gh = h @ U + brec
        if probe is not None:
            gh = gh + probe[:, t]
        z = torch.sigmoid(gx[:, t, :u] + gh[:, :u])
        r = torch.sigmoid(gx[:, t, u:2 * u] + gh[:, u:2 * u])
        hh = torch.tanh(gx[:, t, 2 * u:] + r * gh[:, 2 * u:])
        h = z * h + (1 - z) * hh
        hs[t] = h
        for k, v in (("z", z), ("r", r), ("hh", hh), ("gh_h", gh[:, 2 * u:])):
            kept[k][t] = v
    if aux is not None:
        aux.update({k: torch.stack(v, 1).detach() for k, v in kept.items()})
    return torch.stack(hs, 1)


def lstm_direction(x, kernel, rec_kernel, bias, reverse: bool):
    return lstm_recurrence(x @ kernel + bias, rec_kernel, reverse)[0]


def merge(hf, hb, mode: str):
    """tf.keras.layers.Bidirectional(merge_mode)"""
    if mode == "mul":
        return hf * hb
    if mode == "concat":
        return torch.cat([hf, hb], -1)
    if mode == "ave":
        return (hf + hb) / 2
    if mode == "sum":
        return hf + hb
    raise ValueError(mode)


# ---------------------------------------------------------------- recurrence-level cases (seld_rnn_lstm_*, seld_rnn_gru_*)
FWD_CHUNK, BWD_CHUNK = 16, 8      # the kernels' staging chunks (steps)
LSTM_CASES = [(1, 1), (2, 10), (3, 60)] + [(2, s) for s in (BWD_CHUNK - 1, BWD_CHUNK, BWD_CHUNK + 1, FWD_CHUNK - 1, FWD_CHUNK, FWD_CHUNK + 1, 53)]
UNI_CASE = (3, 17)
SATURATED = (2, 10, 8.0)          # inputs x 8: |z| far in the gates' flat ends
GRU_DH_CASES = [(2, 10), (1, 1)]
GRU_MUL_CASE = (3, 60)
# tests/test_gru_gpu.py: one below, at and one above one and two chunks of both GRU kernels; 53: a ragged tail behind 3 forward / 6 backward chunks
GRU_EDGE_S = (2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 53)
GRU_EDGE_CASES = [(2, s) for s in GRU_EDGE_S] + [(3, 53)]
GRU_BPTT_S = (8, 9, 17, 53)       # the backward kernels alone, on the oracle's own forward values
# recurrent dropout.  Keras scales the masked state by 1 / (1 - rate) at every step: at rate 0.5 |h| grows without bound along the sequence (1.7e4 at
# S = 17) and no fp32 evaluation stays near fp64, so the rate is 0.2 (tests/test_rnn_cpu.py holds |h| <= 4 and the fp32 margin for every case here)
GRU_DROP_RATE = 0.2
GRU_DROP_CASES = [(3, s) for s in (1, 9, 17, 33, 53)]
GRU_DROP_AT_CHUNKS = [(2, s) for s in (8, 16, 32)]      # the same at the lengths that are whole chunks of both kernels
GRU_DROP_BPTT_CASES = [(3, s) for s in GRU_BPTT_S]
GRU_BATCH_CASE = (5, 17)          # every clip of a batch against that clip alone
GRU_SMALLER_BATCH = (2, 17, 3)    # B, S, the batch the buffers are sized for
GRU_SATURATED = (2, 17, 8.0)


def recurrence_inputs(kind: str, B: int, S: int, scale: float = 1.0, seed: int = 0):
    """-> dict of float32 numpy: gx [2][B,S,G], U [2][128,G], dh [2][B,S,128] (+ brec [2][G] for the GRU); index 0 = forward, 1 = backward direction"""
    G = 512 if kind == "lstm" else 384
    rng = np.random.default_rng([B, S, G, seed])
    d = {"gx": f32(scale * rng.standard_normal((2, B, S, G))), "U": f32(rng.standard_normal((2, U_, G)) / math.sqrt(U_)),
         "dh": f32(rng.standard_normal((2, B, S, U_)))}
    if kind == "gru":
        d["brec"] = f32(0.1 * rng.standard_normal((2, G)))
    return d


def lstm_reference(ins, dtype=torch.float64, dirs=(0, 1)):
    """-> {h, c, dgx: [per direction] numpy}"""
    out = {"h": [], "c": [], "dgx": []}
    for d in dirs:
        gx = torch.tensor(ins["gx"][d], dtype=dtype, requires_grad=True)
        h, c = lstm_recurrence(gx, torch.tensor(ins["U"][d], dtype=dtype), bool(d))
        (g,) = torch.autograd.grad((h * torch.tensor(ins["dh"][d], dtype=dtype)).sum(), gx)
        out["h"].append(h.detach().numpy()); out["c"].append(c.detach().numpy()); out["dgx"].append(g.numpy())
    return out


def gru_drop_masks(B: int, rate: float, seed: int = 0):
    """-> float32 [2][B,128], 0 | 1 / (1 - rate): seeded numpy draws, one per direction (the mask values are an INPUT of the dropout kernels; the
    library's own Philox draws are tests/test_model_gpu.py's subject)"""
    rng = np.random.default_rng([B, U_, int(round(rate * 1000)), seed])
    return f32(np.stack([(rng.random((B, U_)) >= rate) for _ in (0, 1)]) / (1.0 - rate))


GRU_SAVED = ("z", "r", "hh", "gh_h")      # the planes of the kernels' saved gates [t][unit][4]


def gru_reference(ins, dtype=torch.float64, dirs=(0, 1), dh=None, rec_mask=None, mul=False):
    """-> {h, dgx, dgh, z, r, hh, gh_h: [per direction] numpy}; dh: the output gradients to use instead of ins['dh'].  rec_mask [2][B,128]: recurrent
    dropout (see gru_recurrence), adds hm = h * rec_mask.  mul: the objective is (h_f h_b dout).sum() with dout = ins['dh'][0], the 'mul' merge of
    seld_k_gru_bwd, and out = [h_f h_b] is returned too"""
    out = {k: [] for k in ("h", "dgx", "dgh") + GRU_SAVED}
    hs, leaves = [], []
    for d in dirs:
        gx = torch.tensor(ins["gx"][d], dtype=dtype, requires_grad=True)
        probe = torch.zeros_like(gx, requires_grad=True)
        aux = {}
        m = None if rec_mask is None else torch.tensor(rec_mask[d], dtype=dtype)
        h = gru_recurrence(gx, torch.tensor(ins["U"][d], dtype=dtype), torch.tensor(ins["brec"][d], dtype=dtype), bool(d), probe, m, aux)
        hs.append(h); leaves += [gx, probe]
        out["h"].append(h.detach().numpy())
        for k in GRU_SAVED:
            out[k].append(aux[k].numpy())
        if m is not None:
            out.setdefault("hm", []).append((h.detach() * m[:, None, :]).numpy())
    if mul:
        assert tuple(dirs) == (0, 1) and dh is None
        y = hs[0] * hs[1]
        out["out"] = [y.detach().numpy()]
        grads = torch.autograd.grad((y * torch.tensor(ins["dh"][0], dtype=dtype)).sum(), leaves)
    else:
        grads = torch.autograd.grad(sum((h * torch.tensor((ins["dh"] if dh is None else dh)[d], dtype=dtype)).sum() for h, d in zip(hs, dirs)), leaves)
    out["dgx"], out["dgh"] = [g.numpy() for g in grads[0::2]], [g.numpy() for g in grads[1::2]]
    return out


def gru_saved(ref, i: int):
    """the saved-gates tensor [B,S,128,4] of direction entry i of a gru_reference result, as the kernels lay it out"""
    return np.stack([ref[k][i] for k in GRU_SAVED], -1)


def gru_pieces(got, ref):
    """everything in `got` beside its reference, per direction entry and PER GATE BLOCK, so that a small block cannot hide behind a large one: h, hm,
    out whole; dgx, dgh by their z | r | h thirds; saved [B,S,128,4] by its four planes against ref's z, r, hh, gh_h.  -> [(name, got, ref)]"""
    res = []
    for k, arrs in got.items():
        for i, a in enumerate(arrs):
            a = np.asarray(a)
            if k in ("h", "hm", "out"):
                res.append((f"{k}[{i}]", a, ref[k][i]))
            elif k in ("dgx", "dgh"):
                for g, gate in enumerate("zrh"):
                    res.append((f"{k}[{i}].{gate}", a[..., g * U_:(g + 1) * U_], ref[k][i][..., g * U_:(g + 1) * U_]))
            elif k == "saved":
                a = a.reshape(ref["z"][i].shape + (4,))
                for g, plane in enumerate(GRU_SAVED):
                    res.append((f"saved[{i}].{plane}", a[..., g], ref[plane][i]))
            else:
                raise KeyError(k)
    for name, a, b in res:
        assert a.shape == np.asarray(b).shape, f"{name}: {a.shape} against {np.asarray(b).shape}"
    return res


def gru_compare(tag, got, ref, tol):
    """helpers.check (max|d| / max|ref| <= tol, finite) on every piece of gru_pieces(got, ref); every piece is measured and printed before the
    failures are raised together.  -> {piece: error}"""
    from helpers import check, rel_err
    bad = []
    for name, a, b in gru_pieces(got, ref):
        try:
            check(f"{tag} {name}", a, b, tol)
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, "; ".join(bad)
    return {name: rel_err(a, b) for name, a, b in gru_pieces(got, ref)}


def merge_inputs(rows: int, units: int, mode: str):
    rng = np.random.default_rng([rows, units, MERGES.index(mode)])
    w = 2 * units if mode == "concat" else units
    return f32(rng.standard_normal((rows, units))), f32(rng.standard_normal((rows, units))), f32(rng.standard_normal((rows, w)))


def merge_reference(hf, hb, dout, mode, dtype=torch.float64):
    a, b = (torch.tensor(v, dtype=dtype, requires_grad=True) for v in (hf, hb))
    y = merge(a, b, mode)
    ga, gb = torch.autograd.grad((y * torch.tensor(dout, dtype=dtype)).sum(), (a, b))
    return y.detach().numpy(), ga.numpy(), gb.numpy()


# ---------------------------------------------------------------- the block and the stage
def is_lstm(cfg):
    return cfg.get("rnn_type", "GRU") != "GRU"      # modules.py:334-337: anything but 'GRU' is an LSTM


def out_dim(cfg):
    return 2 * int(cfg["units"]) if cfg.get("bidirectional", True) and cfg.get("merge_mode", "mul") == "concat" else int(cfg["units"])


def block_specs(D: int, cfg: dict, prefix: str):
    u = int(cfg["units"])
    G = (4 if is_lstm(cfg) else 3) * u
    names = [f"{prefix}.fwd", f"{prefix}.bwd"] if cfg.get("bidirectional", True) else [prefix]
    tr = []
    for n in names:
        tr += [(f"{n}.kernel", (D, G)), (f"{n}.recurrent_kernel", (u, G)), (f"{n}.bias", (G,) if is_lstm(cfg) else (2, G))]
    return tr


def stage_specs(D: int, cfg: dict, depth: int, prefix: str = "rnn"):
    tr = []
    for i in range(depth):
        tr += block_specs(D, cfg, f"{prefix}{i}")
        D = out_dim(cfg)
    return tr


def block_forward(x, w, cfg: dict, prefix: str):
    """x [B,S,D] -> [B,S,out_dim]"""
    names = [f"{prefix}.fwd", f"{prefix}.bwd"] if cfg.get("bidirectional", True) else [prefix]
    hs = []
    for d, n in enumerate(names):
        k, r, b = w[f"{n}.kernel"], w[f"{n}.recurrent_kernel"], w[f"{n}.bias"]
        hs.append(lstm_direction(x, k, r, b, bool(d)) if is_lstm(cfg) else O.gru_direction(x, k, r, b, bool(d)))
    return merge(hs[0], hs[1], cfg.get("merge_mode", "mul")) if len(hs) == 2 else hs[0]


def stage_forward(x, w, cfg: dict, depth: int, prefix: str = "rnn"):
    for i in range(depth):
        x = block_forward(x, w, cfg, f"{prefix}{i}")
    return x


def random_stage_weights(D: int, cfg: dict, depth: int, seed: int, prefix: str = "rnn"):
    """glorot-uniform kernels (the recurrent ones too: not orthogonal, so that nothing cancels), biases of 0.05 sigma"""
    return T.random_block_weights(stage_specs(D, cfg, depth, prefix), seed)


def _c(**kw):
    return dict({"units": 128, "dropout_rate": 0.0}, **kw)


# name -> (B, S, D, depth (None: RNN_block), config)
STAGE_CASES = {
    "lstm concat": (2, 12, 40, None, _c(rnn_type="LSTM", merge_mode="concat")),
    "lstm mul": (2, 12, 40, None, _c(rnn_type="LSTM", merge_mode="mul")),
    "gru ave": (2, 12, 40, None, _c(rnn_type="GRU", merge_mode="ave")),
    "gru unidirectional": (2, 12, 40, None, _c(rnn_type="GRU", bidirectional=False, merge_mode=None)),
    "lstm stage depth 2 concat": (2, 12, 40, 2, _c(rnn_type="LSTM", merge_mode="concat", depth=2)),
    "reference test_RNN_stage": (2, 10, 128, 3, _c(rnn_type="LSTM", merge_mode="concat", depth=3, bidirectional=True)),
}
# the reference's three test configurations (modules_test.py:46-73, 226-242)
REFERENCE_CONFIGS = [
    ({"depth": 3, "units": 64, "bidirectional": True, "merge_mode": "ave", "rnn_type": "GRU", "dropout_rate": 0.3}, True),
    ({"depth": 3, "units": 64, "bidirectional": True, "merge_mode": "concat", "rnn_type": "LSTM", "dropout_rate": 0.}, True),
    ({"units": 64, "bidirectional": False, "merge_mode": None, "rnn_type": "GRU", "dropout_rate": 0.3}, False),
]


def stage_reference(B, S, D, depth, cfg, seed, dtype=torch.float64):
    """-> dict: x, dy, w (numpy inputs), out, dx, grad, specs"""
    n = 1 if depth is None else depth
    tr = stage_specs(D, cfg, n)
    w = random_stage_weights(D, cfg, n, seed)
    rng = np.random.default_rng(seed)
    x, dy = f32(rng.standard_normal((B, S, D))), f32(rng.standard_normal((B, S, out_dim(cfg))))
    fw = torch.tensor(w, dtype=dtype, requires_grad=True)
    xt = torch.tensor(x, dtype=dtype, requires_grad=True)
    y = stage_forward(xt, O.unflatten(fw, tr), cfg, n)
    gw, gx = torch.autograd.grad((y * torch.tensor(dy, dtype=dtype)).sum(), (fw, xt))
    return {"x": x, "dy": dy, "w": w, "out": y.detach().numpy(), "dx": gx.numpy(), "grad": gw.numpy(), "specs": tr}


# ---------------------------------------------------------------- models.seldnet with a mother FIRST block and SECOND = RNN_block / RNN_stage
def _depth(model_config: dict) -> int:
    if model_config["SECOND"] == "RNN_stage":
        return int(model_config["SECOND_ARGS"]["depth"])
    if model_config["SECOND"] == "RNN_block":
        return 1
    raise ValueError("rnn_oracle restates RNN_block / RNN_stage as SECOND")


MODEL_INPUT = (2, 50, 64, 7)


def model_case(seldnet_config: dict, stage_first: dict) -> dict:
    """FIRST = one mother_block of tests/test_modules_gpu.STAGE_FIRST's shape with 8 + 8 filters, SECOND = a two-block LSTM RNN_stage merged by
    concatenation (the heads read 256 features)"""
    cfg = copy.deepcopy(seldnet_config)
    first = dict(copy.deepcopy(stage_first), filters0=8, filters1=8)
    first.pop("depth", None)
    cfg["FIRST"], cfg["FIRST_ARGS"] = "mother_block", first
    cfg["SECOND"] = "RNN_stage"
    cfg["SECOND_ARGS"] = {"depth": 2, "units": 128, "bidirectional": True, "merge_mode": "concat", "rnn_type": "LSTM", "dropout_rate": 0.0}
    return cfg


def _head_less(model_config: dict) -> dict:
    """oracle.modules_oracle sizes the heads' first layer from its own recurrent stage: an empty one, and FIRST's width replaced below"""
    return T._gru_less(model_config)


def variable_specs(model_config: dict, input_shape):
    gl = _head_less(model_config)
    tr, nt = M.variable_specs(gl, input_shape)
    shape = CF._first_out(model_config, input_shape)
    n_first = next(i for i, (n, _) in enumerate(tr + [("sed.", ())]) if n.startswith(("sed.", "doa.")))
    sa = model_config["SECOND_ARGS"]
    mid = stage_specs(shape[1] * shape[2], sa, _depth(model_config))
    heads, a = [], None
    for n, s in tr[n_first:]:      # the heads read the stage's out_dim, not FIRST's width: the first kernel of each head
        if n.endswith("kernel") and a != n.split(".")[0]:
            a = n.split(".")[0]
            s = s[:-2] + (out_dim(sa), s[-1])
        heads.append((n, s))
    return tr[:n_first] + mid + heads, nt


def random_weights(model_config: dict, input_shape, seed: int = 0):
    tr, nt = variable_specs(model_config, input_shape)
    w0, st0 = M.random_weights(_head_less(model_config), input_shape, seed)
    tr0, _ = M.variable_specs(_head_less(model_config), input_shape)
    d0 = {n: (w0[o:o + int(np.prod(s))], s) for (n, s), o in zip(tr0, np.cumsum([0] + [int(np.prod(s)) for _, s in tr0])[:-1])}
    rest = T.random_block_weights([(n, s) for n, s in tr if n not in d0 or d0[n][1] != s], seed + 1)
    out, off = [], 0
    for n, s in tr:
        k = int(np.prod(s))
        if n in d0 and d0[n][1] == s:
            out.append(d0[n][0])
        else:
            out.append(rest[off:off + k])
            off += k
    return np.concatenate(out).astype(np.float32), st0


def forward(model_config: dict, w, st, x, training: bool):
    """-> (sed, doa, new_state)"""
    new_st = dict(st)
    h = x
    for d, cfg in enumerate(M.first_configs(model_config)):
        h = M.mother_block_forward(cfg, w, st, new_st, h, training, f"mb{d}")
    B, S = h.shape[0], h.shape[1]
    h = h.reshape(B, S, -1)          # layers.force_1d_inputs (layers.py:41-47)
    h = stage_forward(h, w, model_config["SECOND_ARGS"], _depth(model_config))
    sp = M._tail_spec(_head_less(model_config))
    outs = []
    for head, units, act, hact in (("sed", sp.sed_units, torch.sigmoid, M.ACTS[sp.sed_dense_act]), ("doa", sp.doa_units, torch.tanh, M.ACTS[sp.doa_dense_act])):
        a = h
        for j in range(len(units)):
            a = hact(a @ w[f"{head}.dense{j}.kernel"][0] + w[f"{head}.dense{j}.bias"])
        outs.append(act(a @ w[f"{head}.out.kernel"] + w[f"{head}.out.bias"]))
    return outs[0], outs[1], new_st


def train_step(model_config: dict, input_shape, flat_w, flat_state, x, y_sed, y_doa, *, doa_loss="MSE", loss_weight=(1.0, 1000.0), lr=1e-3,
               step=1, dtype=torch.float64):
    """train.trainstep (train.py:22-36) -> dict(sed, doa, sloss, dloss, grad, new_w, new_state), all numpy"""
    tr, nt = variable_specs(model_config, input_shape)
    fw = torch.tensor(np.asarray(flat_w), dtype=dtype, requires_grad=True)
    wd = O.unflatten(fw, tr)
    sd = O.unflatten(torch.tensor(np.asarray(flat_state), dtype=dtype), nt)
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype)
    sed, doa, new_st = forward(model_config, wd, sd, t(x), True)
    obj, sloss, dloss = O.losses_and_objective(sed, doa, t(y_sed), t(y_doa), doa_loss, loss_weight)
    (g,) = torch.autograd.grad(obj, fw)
    new_w, _, _ = O.adam_update(fw.detach(), g, torch.zeros_like(fw), torch.zeros_like(fw), step, lr=lr)
    ns = torch.cat([new_st[n].detach().reshape(-1) for n, _ in nt]) if nt else torch.zeros(0, dtype=dtype)
    return {"sed": sed.detach().numpy(), "doa": doa.detach().numpy(), "sloss": sloss.detach().numpy(), "dloss": dloss.detach().numpy(),
            "grad": g.numpy(), "new_w": new_w.numpy(), "new_state": ns.numpy()}


def test_step(model_config: dict, input_shape, flat_w, flat_state, x, y_sed, y_doa, *, doa_loss="MSE", loss_weight=(1.0, 1000.0), dtype=torch.float64):
    tr, nt = variable_specs(model_config, input_shape)
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype)
    with torch.no_grad():
        sed, doa, _ = forward(model_config, O.unflatten(t(flat_w), tr), O.unflatten(t(flat_state), nt), t(x), False)
        _, sloss, dloss = O.losses_and_objective(sed, doa, t(y_sed), t(y_doa), doa_loss, loss_weight)
    return {"sed": sed.numpy(), "doa": doa.numpy(), "sloss": sloss.numpy(), "dloss": dloss.numpy()}
