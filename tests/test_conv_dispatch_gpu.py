"""``dy_conv2d_nhwc``'s dispatch as executed, against tests/golden/conv_dispatch.json (tools/make_conv_dispatch_golden.py recorded it on the
commit before the routing rules moved into one place each, and says what the cases are): per single ``conv2d`` launch the kernel that ran,
the statistics slots it reported and a SHA-256 of the output bytes — or the exception type of a refused call."""
import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_conv_dispatch_golden", os.path.join(ROOT, "tools", "make_conv_dispatch_golden.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)
TABLE = G.load_table()


def test_the_table_holds_every_case_of_the_sweep():
    assert [row[0] for row in TABLE] == G.all_cases()


@pytest.mark.parametrize("spec,want", TABLE, ids=[f"{row[0][0]}-{row[0][1]}" for row in TABLE])
def test_same_kernel_same_slots_same_bytes(spec, want, device):
    assert G.run_case(spec, device) == want
