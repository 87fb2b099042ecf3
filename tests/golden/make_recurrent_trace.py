"""Generates tests/golden/recurrent_trace.json: every call the recurrent blocks of seld_amd/modules.py (RNN_block, RNN_stage,
bidirectional_GRU_block) make into the library, in order and with canonical arguments, for the configurations of CASES — a training forward,
its backward, then an inference forward, each on a runtime built on the CPU whose library is a recorder (no device, no kernel runs).
tests/test_recurrent_trace_cpu.py records the same cases with the same recorder and compares entry by entry, so the fixture pins "the same
launches, in the same order, with the same arguments" across a rewrite of the blocks' Python.

Run from the repo root, AT THE COMMIT WHOSE LAUNCHES ARE TO BE KEPT (uses _build_second, Stage.forward / backward and _Rt only):
    python tests/golden/make_recurrent_trace.py

Canonical arguments (they survive renames of the blocks' attributes):
  * a pointer into the runtime's parameters / gradients: ["w" | "g", variable name, float offset inside the variable];
  * any other pointer: [k, float offset], k = the rank of first appearance of its storage in that case's trace;
  * NULL (and the stream): None;  integers as they are;  floats through float(np.float32(.))."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

B, S, D = 2, 3, 8      # the recorder ignores sizes; the cells' input masks need D % 4 == 0
PATH = os.path.join(ROOT, "tests", "golden", "recurrent_trace.json")


def _cases():
    """name -> (SECOND kind, its arguments, runtime flags)"""
    out = {}
    plain = [(f"gru_bi_{m}", {"units": 128, "merge_mode": m}) for m in ("mul", "concat", "ave", "sum")]
    plain += [("gru_uni", {"units": 128, "bidirectional": False}),
              ("lstm_bi_concat", {"units": 128, "rnn_type": "LSTM", "merge_mode": "concat"}),
              ("lstm_uni", {"units": 128, "rnn_type": "LSTM", "bidirectional": False})]
    for name, cfg in plain:
        out[f"rnn_{name}"] = ("RNN_block", cfg, {})
    for name, cfg in plain:
        out[f"rnn_{name}_drop"] = ("RNN_block", dict(cfg, dropout_rate=0.25), {"dropout": True})
    for u in (5, 64, 256):
        out[f"rnn_gru_u{u}_bi_sum"] = ("RNN_block", {"units": u, "merge_mode": "sum"}, {"any_units": True})
        out[f"rnn_gru_u{u}_uni"] = ("RNN_block", {"units": u, "bidirectional": False}, {"any_units": True})
    out["rnn_gru_u128_any"] = ("RNN_block", {"units": 128}, {"any_units": True})
    out["rnn_stage_lstm_mul"] = ("RNN_stage", {"units": 128, "depth": 2, "rnn_type": "LSTM", "merge_mode": "mul"}, {})
    out["gru_block"] = ("bidirectional_GRU_block", {"units": [128, 128]}, {})
    out["gru_block_u24_128"] = ("bidirectional_GRU_block", {"units": [24, 128]}, {"any_units": True})
    out["gru_block_drop"] = ("bidirectional_GRU_block", {"units": [128, 128], "dropout_rate": 0.2}, {"dropout": True})
    return out


CASES = _cases()


class _Ptr:
    """what the recording runtime's p() hands to the library in place of an address"""

    def __init__(self, t):
        self.t = t


class Recorder:
    """stands in for the library of one runtime: every entry appends (name, canonical arguments) and returns 0 (a *_scratch size: 1)"""

    def __init__(self, rt):
        self.rt, self.calls, self.seen = rt, [], []      # seen: the storages in order of first appearance (the tensors keep them alive)

    def _pointer(self, t):
        rt = self.rt
        base = t.untyped_storage().data_ptr()
        off = (t.data_ptr() - base) // 4
        for tag, store in (("w", rt.params), ("g", rt.grads)):
            if store is not None and base == store.untyped_storage().data_ptr():
                for name, o, sh in rt.variables:
                    if o <= off < o + int(np.prod(sh)):
                        return [tag, name, off - o]
                raise AssertionError(f"a pointer {off} floats into the {tag} store belongs to no variable")
        for k, s in enumerate(self.seen):
            if s.untyped_storage().data_ptr() == base:
                return [k, off]
        self.seen.append(t)
        return [len(self.seen) - 1, off]

    def _canon(self, a):
        if a is None or (hasattr(a, "value") and a.value is None):
            return None
        if isinstance(a, _Ptr):
            return self._pointer(a.t)
        if isinstance(a, (bool, int, np.integer)):
            return int(a)
        if isinstance(a, (float, np.floating)):
            return float(np.float32(a))
        raise AssertionError(f"an argument of type {type(a).__name__}")

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append([name, [self._canon(a) for a in args]])
            return 1 if name.endswith("_scratch") else 0
        return entry


def record(kind, cfg, flags):
    """the calls of one case: a training forward, its backward, an inference forward"""
    from seld_amd import modules as M
    rt = M._Rt(torch.device("cpu"))
    for k, v in flags.items():
        setattr(rt, k, v)
    st = M._build_second(kind, rt, cfg, S, D, B)
    rt.finalize()
    rec = Recorder(rt)
    rt.lib, rt.st, rt.p = rec, (lambda: None), (lambda t: _Ptr(t) if t is not None else None)
    x = torch.zeros(B * S, D)
    if rt.dropout:
        rt.next_draws()
    y = st.forward(x, B, True)
    st.backward(torch.zeros_like(y), B)
    st.forward(x, B, False)
    return rec.calls


def record_all():
    return {name: record(*case) for name, case in CASES.items()}


if __name__ == "__main__":
    traces = record_all()
    with open(PATH, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in traces.items()) + "\n}\n")
    print(PATH, os.path.getsize(PATH), "bytes,", sum(len(v) for v in traces.values()), "calls in", len(traces), "cases")
