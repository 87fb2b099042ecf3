"""What the recurrent blocks (RNN_block, RNN_stage, bidirectional_GRU_block: modules._Recurrent) ask of the library, without a device: every
case of tests/golden/make_recurrent_trace.py runs a training forward, its backward and an inference forward on a CPU runtime whose library is
that file's recorder, and the calls — names, order, canonical arguments — must be those of tests/golden/recurrent_trace.json, recorded before
the blocks' three call paths became one."""
import importlib.util
import json
import os

import pytest

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_recurrent_trace", os.path.join(HERE, "make_recurrent_trace.py"))
T = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(T)

with open(T.PATH) as _f:
    GOLDEN = json.load(_f)


def test_the_fixture_holds_the_case_list():
    assert list(GOLDEN) == list(T.CASES)
    assert os.path.getsize(T.PATH) < 100 * 1024


@pytest.mark.parametrize("name", list(T.CASES))
def test_calls_are_those_recorded(seld_lib, name):
    got = json.loads(json.dumps(T.record(*T.CASES[name])))      # tuples -> lists, as the fixture went through
    want = GOLDEN[name]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{name}: call {i}"
    assert len(got) == len(want), f"{name}: {len(got)} calls, recorded {len(want)}"
    names = {c[0] for c in got}
    assert any(n.startswith(("seld_rnn_", "seld_m_gru_")) for n in names) and "seld_m_gemm_tn" in names
