"""fp64 restatement (torch, CPU) of the recurrent kinds under Keras dropout / recurrent_dropout (reference modules.py:312-315, 338-340 pass
dropout_rate as both), on top of tests/rnn_oracle.py (the cells, the merges, the seeded cases) and oracle.seldnet_oracle's Philox (the masks
are the library's draws).  A helper, not a test file: tests/test_rnn_dropout_cpu.py pins it, tests/test_rnn_dropout_gpu.py holds the device to it.

Each cell — each direction of a Bidirectional, each block of a stage — owns an input mask im [B, D] and a state mask rm [B, 128] of
0 | 1 / (1 - rate), constant over the sequence.  Restated from the published Keras source (the reference pins none of it):
  GRU   GRUCell.call, implementation 2, reset_after=True: oracle.seldnet_oracle.gru_direction(in_mask, rec_mask) / rnn_oracle.gru_recurrence(rec_mask)
  LSTM  LSTMCell.call, implementation 2 (tf.keras.layers.LSTM's default): x_t * im goes into the input projection;
        z = gx_t + (h_prev * rm) U;  c' = f c + i g (c is never masked);  h' = o tanh(c') (emitted unmasked)
Draw streams of block `index` of its stage at training step `step` (seld_amd.modules._Recurrent): layer = 4096 + 32 index + site, site 0 / 1 =
the forward direction's input / state mask, 2 / 3 = the backward direction's; element e of the row-major [B, D] / [B, 128] mask is uniform e."""
import numpy as np
import torch

import dropout_oracle as DO
import rnn_oracle as R
from oracle import modules_oracle as M
from oracle import seldnet_oracle as O

U_ = 128
LSTM_RATES = (0.2, 0.5)
# (1, 1); B = 3 with S one below, at and one above the backward (8) and forward (16) staging chunks; 53: a ragged tail
LSTM_DROP_CASES = [(1, 1)] + [(3, s) for s in (R.BWD_CHUNK - 1, R.BWD_CHUNK, R.BWD_CHUNK + 1, R.FWD_CHUNK - 1, R.FWD_CHUNK, R.FWD_CHUNK + 1, 53)]
LSTM_BATCH_CASE = (5, 17)          # every clip of a batch against that clip alone
LSTM_SMALLER_BATCH = (2, 17, 3)    # B, S, the batch the buffers are sized for


# ---------------------------------------------------------------- the LSTM cell under recurrent dropout
def lstm_recurrence(gx, U, reverse: bool, rec_mask=None):
    """rnn_oracle.lstm_recurrence with the state mask rec_mask [B,u] -> (h, c, acts [B,S,u,4] = i f g o)"""
    B, S, _ = gx.shape
    u = U.shape[0]
    h, c = gx.new_zeros(B, u), gx.new_zeros(B, u)
    hs, cs, av = [None] * S, [None] * S, [None] * S
    for t in (range(S - 1, -1, -1) if reverse else range(S)):
        z = gx[:, t] + (h if rec_mask is None else h * rec_mask) @ U
        i, f, g, o = torch.sigmoid(z[:, :u]), torch.sigmoid(z[:, u:2 * u]), torch.tanh(z[:, 2 * u:3 * u]), torch.sigmoid(z[:, 3 * u:])
        c = f * c + i * g
        h = o * torch.tanh(c)
        hs[t], cs[t], av[t] = h, c, torch.stack([i, f, g, o], -1)
    return torch.stack(hs, 1), torch.stack(cs, 1), torch.stack(av, 1)


def lstm_reference(ins, masks=None, dtype=torch.float64, dirs=(0, 1), with_dU=False):
    """R.recurrence_inputs('lstm') and masks [2][B,128] (None: no dropout) -> {h, c, saved, dgx (, dU): [per direction entry] numpy}"""
    out = {"h": [], "c": [], "saved": [], "dgx": [], "dU": []}
    for d in dirs:
        gx = torch.tensor(ins["gx"][d], dtype=dtype, requires_grad=True)
        U = torch.tensor(ins["U"][d], dtype=dtype, requires_grad=True)
        m = None if masks is None else torch.tensor(masks[d], dtype=dtype)
        h, c, av = lstm_recurrence(gx, U, bool(d), m)
        g, gU = torch.autograd.grad((h * torch.tensor(ins["dh"][d], dtype=dtype)).sum(), (gx, U))
        for k, v in (("h", h), ("c", c), ("saved", av), ("dgx", g), ("dU", gU)):
            out[k].append(v.detach().numpy())
    if not with_dU:
        del out["dU"]
    return out


def shifted(h, d):
    """h_prev of direction d: h[t-1] (forward) / h[t+1] (backward), zero outside the sequence"""
    hp = np.zeros_like(h)
    if d == 0:
        hp[:, 1:] = h[:, :-1]
    else:
        hp[:, :-1] = h[:, 1:]
    return hp


def lstm_direction(x, kernel, rec_kernel, bias, reverse: bool, in_mask=None, rec_mask=None):
    if in_mask is not None:
        x = x * in_mask[:, None, :]
    return lstm_recurrence(x @ kernel + bias, rec_kernel, reverse, rec_mask)[0]


# ---------------------------------------------------------------- the library's draws
def cell_masks(B: int, D: int, rate: float, index: int, step: int, d: int, dtype=torch.float64, seed: int = DO.SEED):
    """-> (im [B, D], rm [B, 128]) of direction d of block `index` at training step `step`"""
    layer = DO.STREAM0 + 32 * int(index) + 2 * d
    return (O.dropout_mask((B, D), DO.rate32(rate), seed, layer, step, dtype), O.dropout_mask((B, U_), DO.rate32(rate), seed, layer + 1, step, dtype))


def cfg_rate(cfg: dict) -> float:
    return DO.rate32(cfg.get("dropout_rate", 0.0) or 0.0)


# ---------------------------------------------------------------- blocks and stages (RNN_block / RNN_stage / bidirectional_GRU_block)
def _as_rnn(kind: str, cfg: dict):
    """-> (the RNN_block configuration of one block, depth, prefix)"""
    if kind == "bidirectional_GRU_block":
        assert all(int(u) == U_ for u in cfg["units"])
        return {"units": U_, "rnn_type": "GRU", "bidirectional": True, "merge_mode": "mul", "dropout_rate": cfg.get("dropout_rate", 0.0)}, len(cfg["units"]), "gru"
    return cfg, (int(cfg["depth"]) if kind == "RNN_stage" else 1), "rnn"


def block_forward(x, w, cfg: dict, prefix: str, index: int, step):
    """rnn_oracle.block_forward in training at dropout step `step` (None: inference, no masks)"""
    names = [f"{prefix}.fwd", f"{prefix}.bwd"] if cfg.get("bidirectional", True) else [prefix]
    rate = cfg_rate(cfg)
    hs = []
    for d, n in enumerate(names):
        k, r, b = w[f"{n}.kernel"], w[f"{n}.recurrent_kernel"], w[f"{n}.bias"]
        im, rm = cell_masks(x.shape[0], x.shape[2], rate, index, step, d, x.dtype) if step is not None and rate > 0 else (None, None)
        cell = lstm_direction if R.is_lstm(cfg) else O.gru_direction
        hs.append(cell(x, k, r, b, bool(d), in_mask=im, rec_mask=rm))
    return R.merge(hs[0], hs[1], cfg.get("merge_mode", "mul")) if len(hs) == 2 else hs[0]


def stage_forward(x, w, cfg: dict, depth: int, step, prefix: str = "rnn", first_block: int = 0):
    for i in range(depth):
        x = block_forward(x, w, cfg, f"{prefix}{i}", first_block + i, step)
    return x


def _c(**kw):
    return dict({"units": 128}, **kw)


# name -> (kind, B, S, D, config)
STAGE_CASES = {
    "lstm concat": ("RNN_block", 2, 12, 40, _c(rnn_type="LSTM", merge_mode="concat", dropout_rate=0.3)),
    "lstm mul": ("RNN_block", 2, 12, 40, _c(rnn_type="LSTM", merge_mode="mul", dropout_rate=0.3)),
    "gru ave": ("RNN_block", 2, 12, 40, _c(rnn_type="GRU", merge_mode="ave", dropout_rate=0.2)),
    "gru unidirectional": ("RNN_block", 2, 12, 40, _c(rnn_type="GRU", bidirectional=False, merge_mode=None, dropout_rate=0.2)),
    "lstm stage depth 2 concat": ("RNN_stage", 2, 12, 40, _c(rnn_type="LSTM", merge_mode="concat", depth=2, dropout_rate=0.3)),
    "bidirectional_GRU_block": ("bidirectional_GRU_block", 2, 12, 40, {"units": [128, 128], "dropout_rate": 0.2}),
}
STAGE_SEED = 3


def stage_reference(kind, B, S, D, cfg, seed, step, dtype=torch.float64):
    """-> dict: x, dy, w (numpy inputs), out (the training forward at dropout step `step`; None: inference), dx, grad, specs"""
    one, depth, prefix = _as_rnn(kind, cfg)
    tr = R.stage_specs(D, one, depth, prefix)
    w = R.random_stage_weights(D, one, depth, seed, prefix)
    rng = np.random.default_rng(seed)
    x, dy = R.f32(rng.standard_normal((B, S, D))), R.f32(rng.standard_normal((B, S, R.out_dim(one))))
    fw = torch.tensor(w, dtype=dtype, requires_grad=True)
    xt = torch.tensor(x, dtype=dtype, requires_grad=True)
    y = stage_forward(xt, O.unflatten(fw, tr), one, depth, step, prefix)
    gw, gx = torch.autograd.grad((y * torch.tensor(dy, dtype=dtype)).sum(), (fw, xt))
    return {"x": x, "dy": dy, "w": w, "out": y.detach().numpy(), "dx": gx.numpy(), "grad": gw.numpy(), "specs": tr}


# ---------------------------------------------------------------- models.seldnet with SECOND = RNN_stage under dropout
def model_case(seldnet_config: dict, stage_first: dict, rate: float = R.GRU_DROP_RATE) -> dict:
    """rnn_oracle.model_case's FIRST; SECOND = a two-block GRU RNN_stage merged by 'ave' at dropout_rate `rate`"""
    cfg = R.model_case(seldnet_config, stage_first)
    cfg["SECOND_ARGS"] = {"depth": 2, "units": 128, "bidirectional": True, "merge_mode": "ave", "rnn_type": "GRU", "dropout_rate": rate}
    return cfg


def train_step(model_config: dict, input_shape, flat_w, flat_state, x, y_sed, y_doa, *, dropout_step: int, doa_loss="MSE", loss_weight=(1.0, 1000.0),
               dtype=torch.float64):
    """rnn_oracle.train_step with the SECOND stage's cells drawing at `dropout_step` -> dict(sed, doa, sloss, dloss, grad), all numpy"""
    tr, nt = R.variable_specs(model_config, input_shape)
    fw = torch.tensor(np.asarray(flat_w), dtype=dtype, requires_grad=True)
    w = O.unflatten(fw, tr)
    st = O.unflatten(torch.tensor(np.asarray(flat_state), dtype=dtype), nt)
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype)
    new_st = dict(st)
    h = t(x)
    for d, cfg in enumerate(M.first_configs(model_config)):
        h = M.mother_block_forward(cfg, w, st, new_st, h, True, f"mb{d}")
    h = h.reshape(h.shape[0], h.shape[1], -1)
    h = stage_forward(h, w, model_config["SECOND_ARGS"], R._depth(model_config), dropout_step)
    sp = M._tail_spec(R._head_less(model_config))
    outs = []
    for head, units, act, hact in (("sed", sp.sed_units, torch.sigmoid, M.ACTS[sp.sed_dense_act]), ("doa", sp.doa_units, torch.tanh, M.ACTS[sp.doa_dense_act])):
        a = h
        for j in range(len(units)):
            a = hact(a @ w[f"{head}.dense{j}.kernel"][0] + w[f"{head}.dense{j}.bias"])
        outs.append(act(a @ w[f"{head}.out.kernel"] + w[f"{head}.out.bias"]))
    obj, sloss, dloss = O.losses_and_objective(outs[0], outs[1], t(y_sed), t(y_doa), doa_loss, loss_weight)
    (g,) = torch.autograd.grad(obj, fw)
    return {"sed": outs[0].detach().numpy(), "doa": outs[1].detach().numpy(), "sloss": sloss.detach().numpy(), "dloss": dloss.detach().numpy(),
            "grad": g.numpy()}
