"""The eligibility boundaries of the convolution dispatch against tests/golden/conv_accepts.json (tools/make_conv_accepts_golden.py recorded it
on the commit before the rules moved into csrc, and says what the cases are): what ``PackedConv.for_call`` answers on both sides of every
view-size, pitch and alignment limit of the kernels behind DY_WLAYOUT_HALO3X3, and which dense 1x1 shapes are packed for the streaming
kernel.  No GPU; needs the built library."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_conv_accepts_golden", os.path.join(ROOT, "tools", "make_conv_accepts_golden.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)
TABLE = G.load_table()


def test_the_table_holds_every_key_of_the_sweep():
    assert [row[0] for row in TABLE] == G.all_keys()
    assert sum(len(answer) for _, answer in TABLE) > 16000  # one character per case


@pytest.mark.parametrize("key,answer", TABLE, ids=["-".join(str(v) for v in row[0]) for row in TABLE])
def test_every_recorded_answer_reproduces(key, answer):
    """One answer per case, compared character by character: the layout of the pack and "s" / "r" per call form, or the layout per cin."""
    got = G.run_key(key)
    assert len(got) == len(answer)
    wrong = [i for i, (a, b) in enumerate(zip(got, answer)) if a != b]
    assert not wrong, f"{len(wrong)} of {len(answer)} cases differ, the first at index {wrong[0]}: recorded {answer[wrong[0]]}, now {got[wrong[0]]}"
