"""The voice-activity model of the reference, models.spectro_temporal_attention_based_VAD (models.py:105-163), composed from the module
operators of libseld_hip.so (modules.py's layers) and the seld_vad_* kernels of csrc/vad.hip, and the irregular frame window a whole
utterance is scored through (train_vad_baseline.py:76-106, 206-214; vad_dataloader.py:118-123).  There is no CPU or PyTorch fallback.

  SpectroTemporalVAD   x [B, T, F, C] -> (out [B, T, 1], pipe [B, T, 1], score [B, T])
    spectral attention  depth x { Conv2D + BatchNormalization (a), Conv2D + BatchNormalization (b), a * sigmoid(b), MaxPooling2D([1, 2]) }:
                        the tail is seld_vad_gate_pool_fwd / _bwd, or — FUSED_GATE False — seld_m_act, seld_rnn_merge_* (mul) and seld_pool2d_*
    pipe net            2 x { Dense(Np), BatchNormalization, relu, Dropout }, pipe = sigmoid(Dense(1))
    temporal attention  q = BN(Dense(Nt, no bias)(mean over t)), k, v = BN(Dense(Nt, no bias)(x)); seld_vad_tattn_fwd / _bwd apply the sigmoids,
                        the head-fast reshape (column n = d H + h), both softmaxes over time
    post net            Dense(Np), BatchNormalization, relu, Dropout, out = sigmoid(Dense(1))
  loss                  the three outputs' binary cross-entropy against one y [B, T], weighted and summed (models_test.py:59-60): seld_vad_bce
  preprocess_window, seq_to_windows, windows_to_seq, predict_sequence      the reference's names on device tensors (seld_vad_windows / _unwindow)

Variables are in Keras creation order (stage i: conv_a, bn_a, conv_b, bn_b; pipe0, pipe1, pipe_out; query, key, value; post0; out).  Dropout follows
the composed path's rule (modules._Drop): without dropout=True the rate must be present and 0; with it the masks are the library's Philox
draws at layer = DROP_STREAM0 + site, sites 0 and 1 the pipe net, site 2 the post net."""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np
import torch

from . import _lib
from .modules import ACT, BatchNorm, ComposedSeldNet, Dense, Linear, _ConvBN, _Drop, _Rt

CONFIG_DEFAULTS = {"T": 4, "Nc": 16, "fc": 3, "Np": 256, "Nt": 128, "H": 4, "dropout_rate": 0.5}      # models.py:106-113
MAX_NT, MAX_T = 512, 64      # SELD_VAD_MAX_NT, SELD_VAD_MAX_T (include/seld_hip.h)
_SIG, _RELU = ACT["sigmoid"], ACT["relu"]


def check_config(model_config: dict, input_shape, dropout: bool = False) -> dict:
    """-> the configuration with the reference's defaults filled in (depth, Nc, fc, Np, Nt, H as ints, dropout_rate as the fp32 the kernels
    compare with); ValueError, without a device, for everything the model or its kernels refuse"""
    c = dict(CONFIG_DEFAULTS, **{k: v for k, v in model_config.items() if k in CONFIG_DEFAULTS})
    out = {k: int(c[k]) for k in ("T", "Nc", "fc", "Np", "Nt", "H")}
    for k, v in out.items():
        if v < 1 or v != c[k]:
            raise ValueError(f"spectro_temporal_attention_based_VAD: {k} {c[k]!r} must be an integer >= 1")
    if out["Nt"] % out["H"]:
        raise ValueError(f"spectro_temporal_attention_based_VAD: Nt {out['Nt']} is no multiple of H {out['H']}")
    if out["Nt"] > MAX_NT:
        raise ValueError(f"spectro_temporal_attention_based_VAD: Nt {out['Nt']}: the temporal attention kernels take at most {MAX_NT}")
    if len(input_shape) != 4 or min(int(v) for v in input_shape) < 1:
        raise ValueError(f"spectro_temporal_attention_based_VAD: input_shape {tuple(input_shape)!r}: [B, T, F, C], all >= 1")
    if int(input_shape[1]) > MAX_T:
        raise ValueError(f"spectro_temporal_attention_based_VAD: {input_shape[1]} frames: the temporal attention kernels take at most {MAX_T}")
    if int(input_shape[2]) >> out["T"] < 1:
        raise ValueError(f"spectro_temporal_attention_based_VAD: {out['T']} MaxPooling2D([1, 2]) leave nothing of {input_shape[2]} frequency bins")
    if not dropout:
        if "dropout_rate" not in model_config or float(model_config["dropout_rate"]) != 0.0:
            raise ValueError("spectro_temporal_attention_based_VAD: the reference's Dropout draws from TensorFlow's generator, which this path cannot "
                             "reproduce, and the reference's default dropout_rate is 0.5: dropout_rate must be present and 0 — or the caller accepts "
                             "the library's own counter-based draws: dropout=True")
        out["dropout_rate"] = 0.0
    else:
        r = float(np.float32(c["dropout_rate"]))
        if not 0.0 <= r < 1.0:
            raise ValueError(f"spectro_temporal_attention_based_VAD: dropout_rate {c['dropout_rate']!r}: 0 <= dropout_rate < 1")
        out["dropout_rate"] = r
    return out


class _DenseNoBias(Linear):
    """tf.keras.layers.Dense(units, use_bias=False): Linear without the bias variable"""

    def __init__(self, rt: _Rt, name: str, rows: int, K: int, N: int):
        self.rt, self.name, self.K, self.N = rt, name, int(K), int(N)
        rt.var(f"{name}.kernel", (self.K, self.N))
        self.z = rt.empty(rows, self.N)

    def forward(self, x, rows):
        rt = self.rt
        self.a = x
        rt.gemm(x, rt.w(f"{self.name}.kernel"), None, self.z, rows, self.N, self.K)
        return self.z[:rows]

    def backward(self, dz, dx, rows, accumulate=0):
        rt = self.rt
        rt.gemm_tn(self.a, dz, rt.g(f"{self.name}.kernel"), None, rows, self.K, self.N)
        if dx is not None:
            rt.gemm(dz, rt.w(f"{self.name}.kernel"), None, dx, rows, self.K, self.N, transb=1, accumulate=int(accumulate))


class _GatedStage:
    """One spectral-attention stage (models.py:120-122): y = MaxPooling2D([1, 2])(BN(Conv2D(x)) * sigmoid(BN(Conv2D(x)))).  fused: the tail is
    seld_vad_gate_pool_*; otherwise sigmoid, product and pooling are three operators with the gated tensor in memory."""

    def __init__(self, rt: _Rt, name: str, in_shape, filters: int, k: int, B: int, need_dx: bool, fused: bool):
        self.rt, self.fused = rt, bool(fused)
        self.a = _ConvBN(rt, f"{name}.conv_a", f"{name}.bn_a", in_shape, filters, k, (1, 1), B)
        self.b = _ConvBN(rt, f"{name}.conv_b", f"{name}.bn_b", in_shape, filters, k, (1, 1), B)
        self.T, self.W, self.C = int(in_shape[0]), int(in_shape[1]), int(filters)
        self.out_shape = (self.T, self.W // 2, self.C)
        full = (B, self.T, self.W, self.C)
        self.ya, self.yb, self.da, self.db = (rt.empty(*full) for _ in range(4))
        self.y = rt.empty(B, *self.out_shape)
        self.idx = torch.empty((B,) + self.out_shape, dtype=torch.uint8, device=rt.dev)
        self.dx = rt.empty(B, *in_shape) if need_dx else None
        if not self.fused:
            self.sb, self.g, self.dg, self.dsb = (rt.empty(*full) for _ in range(4))

    def tail_forward(self, B, training):
        rt, rows = self.rt, B * self.T
        idx = rt.p(self.idx) if training else None
        if self.fused:
            rt.ck(rt.lib.seld_vad_gate_pool_fwd(rt.p(self.ya), rt.p(self.yb), self.C, rt.p(self.y), idx, rows, self.W, self.C, rt.st()))
        else:
            n = rows * self.W
            rt.act(self.yb[:B], self.sb[:B], _SIG)
            rt.ck(rt.lib.seld_rnn_merge_fwd(rt.p(self.ya), rt.p(self.sb), rt.p(self.g), n, self.C, _lib.SELD_MERGE["mul"], rt.st()))
            rt.ck(rt.lib.seld_pool2d_fwd(rt.p(self.g), rt.p(self.y), idx, B, self.T, self.W, self.C, 1, 2, 0, rt.st()))
        return self.y[:B]

    def tail_backward(self, dy, B):
        rt, rows = self.rt, B * self.T
        if self.fused:
            rt.ck(rt.lib.seld_vad_gate_pool_bwd(rt.p(self.ya), rt.p(self.yb), self.C, rt.p(self.idx), rt.p(dy), rt.p(self.da), rt.p(self.db), rows,
                                                self.W, self.C, rt.st()))
        else:
            n = rows * self.W
            rt.ck(rt.lib.seld_pool2d_bwd(rt.p(dy), rt.p(self.idx), rt.p(self.dg), B, self.T, self.W, self.C, 1, 2, 0, rt.st()))
            rt.ck(rt.lib.seld_rnn_merge_bwd(rt.p(self.dg), rt.p(self.ya), rt.p(self.sb), rt.p(self.da), rt.p(self.dsb), n, self.C,
                                            _lib.SELD_MERGE["mul"], rt.st()))
            rt.act_bwd(self.yb[:B], self.dsb[:B], self.db[:B], _SIG)

    def forward(self, x, B, training):
        self.a.forward(x, self.ya, B, training, 0)
        self.b.forward(x, self.yb, B, training, 0)
        return self.tail_forward(B, training)

    def backward(self, dy, B):
        self.tail_backward(dy, B)
        self.a.backward(self.da, self.dx, B, 0)
        self.b.backward(self.db, self.dx, B, 1)
        return None if self.dx is None else self.dx[:B]


class _DenseBNRelu:
    """Dense(units) -> BatchNormalization -> relu -> Dropout (site) on [B * T, Cin]: the pipe net's and the post net's layer"""

    def __init__(self, rt: _Rt, name: str, T: int, Cin: int, units: int, B: int, drop: _Drop, site: int):
        self.rt, self.T, self.drop, self.site = rt, int(T), drop, int(site)
        self.dense = Dense(rt, f"{name}.dense", B * T, Cin, units)
        self.bn = BatchNorm(rt, f"{name}.bn", (T, 1, units), B)
        self.n, self.h, self.dn, self.dz = (rt.empty(B * T, units) for _ in range(4))

    def forward(self, x, B, training):
        rt, R = self.rt, B * self.T
        self.bn.forward(self.dense.forward(x, R), self.n, B, training, 0)
        rt.act(self.n[:R], self.h[:R], _RELU)
        if self.drop.on:
            self.drop.apply(self.site, self.h[:R], self.h[:R])
        return self.h[:R]

    def backward(self, dh, dx, B):
        """dh [B * T, units] (overwritten where the Dropout draws) -> the variables' gradients and dx"""
        rt, R = self.rt, B * self.T
        if self.drop.on:
            self.drop.apply(self.site, dh, dh)
        rt.act_bwd(self.n[:R], dh, self.dn[:R], _RELU)
        self.bn.backward(self.dn, self.dz, B)
        self.dense.backward(self.dz, dx, R)


class _Projection:
    """Dense(Nt, use_bias=False) -> BatchNormalization on `steps` rows per clip: query (steps 1), key and value (steps T), before the sigmoid"""

    def __init__(self, rt: _Rt, name: str, steps: int, Cin: int, units: int, B: int):
        self.steps = int(steps)
        self.dense = _DenseNoBias(rt, f"{name}.dense", B * steps, Cin, units)
        self.bn = BatchNorm(rt, f"{name}.bn", (steps, 1, units), B)
        self.n, self.dn, self.dz = (rt.empty(B * steps, units) for _ in range(3))

    def forward(self, x, B, training):
        self.bn.forward(self.dense.forward(x, B * self.steps), self.n, B, training, 0)
        return self.n

    def backward(self, dx, B, accumulate=0):
        self.bn.backward(self.dn, self.dz, B)
        self.dense.backward(self.dz, dx, B * self.steps, accumulate)


class SpectroTemporalVAD(ComposedSeldNet):
    """models.spectro_temporal_attention_based_VAD(input_shape = (B, T, F, C), model_config): the weight, gradient and optimizer-slot buffers,
    get / set_weights, save / load_weights and the Dropout counters are ComposedSeldNet's; forward, backward, loss and steps are this model's.
    FUSED_GATE: the spectral tail runs on seld_vad_gate_pool_* (tools/bench_vad.py measures it against the three-operator composition:
    DESIGN.md section 3t); an instance takes `fused_gate` to override it."""
    FUSED_GATE = True

    def __init__(self, input_shape, model_config: dict, device=None, dropout: bool = False, fused_gate=None):
        cfg = self.cfg = check_config(model_config, input_shape, dropout)
        if not torch.cuda.is_available():
            raise RuntimeError("seld_amd needs a HIP device: there is no CPU fallback")
        self._dev = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
        B, T, Fq, Ch = (int(v) for v in input_shape)
        self.input_shape, self.T = (B, T, Fq, Ch), T
        rt = self.rt = _Rt(self._dev)
        rt.dropout = bool(dropout)
        self.lib = rt.lib
        fused = self.FUSED_GATE if fused_gate is None else bool(fused_gate)
        self.drop = _Drop(rt, cfg["dropout_rate"])
        shape = (T, Fq, Ch)
        self.stages = []
        for i in range(cfg["T"]):
            st = _GatedStage(rt, f"sa{i}", shape, cfg["Nc"] << i, cfg["fc"], B, need_dx=i > 0, fused=fused)
            self.stages.append(st)
            shape = st.out_shape
        self.feat_shape = shape
        Np, Nt, R = cfg["Np"], cfg["Nt"], B * T
        fin = shape[1] * shape[2]      # Reshape((T, -1)): feature = f * C + c, the NHWC order
        self.pipe = [_DenseBNRelu(rt, "pipe0", T, fin, Np, B, self.drop, 0), _DenseBNRelu(rt, "pipe1", T, Np, Np, B, self.drop, 1)]
        self.pipe_out = Dense(rt, "pipe_out", R, Np, 1)
        self.query = _Projection(rt, "query", 1, Np, Nt, B)
        self.key = _Projection(rt, "key", T, Np, Nt, B)
        self.value = _Projection(rt, "value", T, Np, Nt, B)
        self.post = _DenseBNRelu(rt, "post0", T, Nt, Np, B, self.drop, 2)
        self.out = Dense(rt, "out", R, Np, 1)
        rt.finalize()
        self.variables, self.state_variables = rt.variables, rt.state_variables
        self.n_params, self.n_state = rt.n_params, rt.n_state
        self.xmean, self.dmean = rt.empty(B, Np), rt.empty(B, Np)
        self.zeros = torch.zeros(B, Np, dtype=torch.float32, device=self._dev)
        self.att, self.datt = rt.empty(R, Nt), rt.empty(R, Nt)
        self.P = rt.empty(B, T, cfg["H"])
        self.dxp, self.dx1, self.dpost = rt.empty(R, Np), rt.empty(R, Np), rt.empty(R, Np)
        self.dfeat = rt.empty(R, fin)
        self.d_out, self.d_pipe, self.d_score, self.dzo, self.dzp = (rt.empty(R) for _ in range(5))
        self.loss_scratch = rt.empty(int(rt.lib.seld_vad_bce_scratch(R)))
        self.adam_step = 0
        self._marks = None
        self._init_weights()

    def summary(self) -> str:
        B, T = self.input_shape[:2]
        lines = [f"SpectroTemporalVAD input {self.input_shape} -> out [B,{T},1], pipe [B,{T},1], score [B,{T}]"]
        lines += [f"  {n:32s} {str(sh):20s} {int(np.prod(sh)):8d}" for n, _, sh in self.variables]
        lines.append(f"Trainable params: {self.n_params}; non-trainable: {self.n_state}")
        text = "\n".join(lines)
        print(text)
        return text

    # ---------------------------------------------------------------- forward / backward
    def _forward(self, x, training: bool):
        rt, cfg = self.rt, self.cfg
        B = x.shape[0]
        R = B * self.T
        if training:
            rt.next_draws()
        self.drop.begin(training)
        h = x
        for st in self.stages:
            h = st.forward(h, B, training)
        feat = h.reshape(R, -1)
        for blk in self.pipe:
            feat = blk.forward(feat, B, training)
        self.xp = feat
        pipe, out, score = rt.empty(B, self.T, 1), rt.empty(B, self.T, 1), rt.empty(B, self.T)
        rt.act(self.pipe_out.forward(feat, R), pipe, _SIG)
        rt.ck(rt.lib.seld_m_mean_hw(rt.p(feat), rt.p(self.xmean), B, self.T, cfg["Np"], rt.st()))
        qn = self.query.forward(self.xmean, B, training)
        kn = self.key.forward(feat, B, training)
        vn = self.value.forward(feat, B, training)
        rt.ck(rt.lib.seld_vad_tattn_fwd(rt.p(qn), rt.p(kn), rt.p(vn), rt.p(self.att), rt.p(score), rt.p(self.P) if training else None, B, self.T,
                                        cfg["Nt"], cfg["H"], rt.st()))
        rt.act(self.out.forward(self.post.forward(self.att[:R], B, training), R), out, _SIG)
        self._score = score
        return out, pipe, score

    def __call__(self, x, training: bool = False):
        return list(self._forward(self._prep(x), bool(training)))

    def _backward(self, B):
        """from the three outputs' gradients (d_out, d_pipe: with respect to the probabilities; d_score) to every variable's gradient"""
        rt, cfg = self.rt, self.cfg
        R = B * self.T
        rt.act_bwd(self.out.z[:R], self.d_out[:R], self.dzo[:R], _SIG)
        self.out.backward(self.dzo, self.dpost, R)
        self.post.backward(self.dpost[:R], self.datt, B)
        q, k, v = self.query, self.key, self.value
        rt.ck(rt.lib.seld_vad_tattn_bwd(rt.p(q.n), rt.p(k.n), rt.p(v.n), rt.p(self.P), rt.p(self._score), rt.p(self.datt), rt.p(self.d_score),
                                        rt.p(q.dn), rt.p(k.dn), rt.p(v.dn), B, self.T, cfg["Nt"], cfg["H"], rt.st()))
        v.backward(self.dxp, B, 0)
        k.backward(self.dxp, B, 1)
        q.backward(self.dmean, B, 0)
        rt.act_bwd(self.pipe_out.z[:R], self.d_pipe[:R], self.dzp[:R], _SIG)
        self.pipe_out.backward(self.dzp, self.dxp, R, 1)
        # the mean over t in front of the query: dxp[b, t, :] += dmean[b, :] / T — seld_m_scale_hw_bwd_dx with a zero scale (0 * xp adds nothing)
        rt.ck(rt.lib.seld_m_scale_hw_bwd_dx(rt.p(self.xp), rt.p(self.zeros), rt.p(self.dmean), rt.p(self.dxp), B, self.T, cfg["Np"], 1, rt.st()))
        self.pipe[1].backward(self.dxp[:R], self.dx1, B)
        self.pipe[0].backward(self.dx1[:R], self.dfeat, B)
        dy = self.dfeat[:R].view(B, *self.feat_shape)
        for st in reversed(self.stages):
            dy = st.backward(dy, B)

    # ---------------------------------------------------------------- loss and steps
    def _label(self, y, B):
        y = torch.as_tensor(y, dtype=torch.float32, device=self._dev).contiguous()
        if tuple(y.shape) != (B, self.T):
            raise ValueError(f"label shape {tuple(y.shape)}: one y [B, T] = {(B, self.T)} for the three outputs")
        return y

    def _loss(self, outs, y, loss_weights: Sequence[float], want_grads: bool):
        """sum_i w_i mean BCE(y, output i) (models_test.py:59-60) -> a device scalar; want_grads: d_out, d_pipe, d_score are written"""
        rt = self.rt
        n = y.numel()
        if len(loss_weights) != 3:
            raise ValueError("loss_weights: one weight per output (out, pipe, score)")
        loss = torch.empty((), dtype=torch.float32, device=self._dev)
        for i, (o, d) in enumerate(zip(outs, (self.d_out, self.d_pipe, self.d_score))):
            rt.ck(rt.lib.seld_vad_bce(rt.p(o), rt.p(y), rt.p(loss), rt.p(d) if want_grads else None, rt.p(self.loss_scratch), n,
                                      float(loss_weights[i]), int(i > 0), rt.st()))
        return loss

    def train_step(self, x, y, optimizer, loss_weights=(1.0, 1.0, 1.0)):
        """one step of model.fit on (x, y [B, T]) -> ([out, pipe, score], loss).  optimizer: train.Adam (seld_m_adam) or trainv2.AdaBelief (the
        AdaBelief of seld_v2_opt without regulariser and clipping: train_vad_baseline.py:47); no host synchronisation"""
        from .trainv2 import AdaBelief
        rt = self.rt
        x = self._prep(x)
        B = x.shape[0]
        y = self._label(y, B)
        belief = isinstance(optimizer, AdaBelief)
        if belief:
            self._v2_get_plan()      # its one-time allocation and copies come before the step's first launch
        outs = self._forward(x, True)
        loss = self._loss(outs, y, loss_weights, True)
        self._backward(B)
        if belief:
            self._v2_opt(optimizer, 0.0, 0.0)
        else:
            self.adam_step += 1
            rt.ck(rt.lib.seld_m_adam(rt.p(rt.params), rt.p(rt.grads), rt.p(rt.adam_m), rt.p(rt.adam_v), self.n_params, optimizer.learning_rate,
                                     optimizer.beta_1, optimizer.beta_2, optimizer.epsilon, self.adam_step, rt.st()))
        return list(outs), loss

    def test_step(self, x, y, loss_weights=(1.0, 1.0, 1.0)):
        x = self._prep(x)
        y = self._label(y, x.shape[0])
        outs = self._forward(x, False)
        return list(outs), self._loss(outs, y, loss_weights, False)

    def train_step_v2(self, *a, **k):
        raise ValueError("the trainv2 recipe (SELD losses) is not this model's: train_step(x, y, optimizer)")


# ---------------------------------------------------------------- the irregular frame window
def preprocess_window(window) -> np.ndarray:
    """vad_dataloader.py:118-123: an int is range(window); the offsets minus their minimum, as int32"""
    w = np.arange(window, dtype=np.int32) if isinstance(window, (int, np.integer)) else np.asarray(window, dtype=np.int32).reshape(-1)
    if w.size < 1:
        raise ValueError("window: at least one offset")
    return (w - w.min()).astype(np.int32)


def _table(window):
    w = np.ascontiguousarray(np.asarray(window, dtype=np.int32).reshape(-1))
    if w.size < 1 or w[0] != 0 or (np.diff(w) < 0).any():
        raise ValueError(f"window {w.tolist()}: preprocess_window's result of sorted offsets (non-decreasing, the first one 0)")
    return w, w.ctypes.data_as(C.POINTER(C.c_int32))


def _stream(t):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def seq_to_windows(seq: torch.Tensor, window) -> torch.Tensor:
    """train_vad_baseline.py:76-86: seq [len, ...] (device, fp32) -> windows [len - max(window), len(window), ...]"""
    w, wp = _table(window)
    seq = seq.to(torch.float32).contiguous()
    n = seq.shape[0] - int(w[-1])
    if n < 1:
        raise ValueError(f"a sequence of {seq.shape[0]} frames holds no window of width {int(w[-1])}")
    D = int(np.prod(seq.shape[1:])) if seq.dim() > 1 else 1
    win = torch.empty((n, w.size) + tuple(seq.shape[1:]), dtype=torch.float32, device=seq.device)
    _lib.check(_lib.load().seld_vad_windows(C.c_void_p(seq.data_ptr()), C.c_void_p(win.data_ptr()), wp, int(w.size), seq.shape[0], D, _stream(seq)))
    return win


def windows_to_seq(windows: torch.Tensor, window) -> torch.Tensor:
    """train_vad_baseline.py:89-106: windows [n, len(window), ...] -> seq [n + max(window), ...], each frame the mean of the windows' values for it"""
    w, wp = _table(window)
    windows = windows.to(torch.float32).contiguous()
    if windows.dim() < 2 or windows.shape[1] != w.size or windows.shape[0] < 1:
        raise ValueError(f"windows shape {tuple(windows.shape)}: [n, {w.size}, ...]")
    D = int(np.prod(windows.shape[2:])) if windows.dim() > 2 else 1
    seq = torch.empty((windows.shape[0] + int(w[-1]),) + tuple(windows.shape[2:]), dtype=torch.float32, device=windows.device)
    _lib.check(_lib.load().seld_vad_unwindow(C.c_void_p(windows.data_ptr()), C.c_void_p(seq.data_ptr()), wp, int(w.size), windows.shape[0], D,
                                             _stream(windows)))
    return seq


def model_out(model, x) -> torch.Tensor:
    """the prediction the recipes score: SpectroTemporalVAD's `out` (the first of its three outputs) or the one tensor a models.vad_architecture
    returns"""
    r = model(x)
    return r[0] if isinstance(r, (list, tuple)) else r


def predict_sequence(model, x, window, batch_size=None) -> torch.Tensor:
    """train_vad_baseline.py:206-214: x [len, F, C] -> windows -> the model's prediction (model_out) in batches -> windows_to_seq: [len, 1]
    (SpectroTemporalVAD) or [len] (a models.vad_architecture whose prediction is [B, Wn])"""
    x = torch.as_tensor(x, dtype=torch.float32).to(model._dev)
    wins = seq_to_windows(x, window)
    bs = model.input_shape[0] if batch_size is None else int(batch_size)
    if not 1 <= bs <= model.input_shape[0]:
        raise ValueError(f"batch_size {batch_size!r}: 1 .. {model.input_shape[0]}, the batch the model was built for")
    outs = [model_out(model, wins[i:i + bs]) for i in range(0, wins.shape[0], bs)]
    return windows_to_seq(torch.cat(outs, dim=0), window)
