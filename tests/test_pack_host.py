"""Host weight packing against tests/golden/conv_pack_table.json (tools/make_pack_golden.py recorded it, and says what the cases are):
every pack of the table comes out byte for byte, and ``conv_pack_plan`` — integers in, no tensor made — names the layout and geometry
of every one of them.  No GPU; needs the built library, like test_host_logic.py::test_packed_weight_layout."""
import functools
import importlib.util
import os

from drone_yolo_amd import hip_ops as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_pack_golden", os.path.join(ROOT, "tools", "make_pack_golden.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)


@functools.lru_cache(maxsize=None)
def _replayed():
    """[(recorded line, the (spec, result) pairs of its shape as packed now)] — packed once for both tests."""
    return [(row, G.run_group(row[0])) for row in G.load_table()]


def test_every_recorded_pack_reproduces_exactly():
    """Per shape, the same SHA-256 over every case's record: layout, geometry, element count and SHA-256 over (w, b, wscale) — or the
    exception type — and what ``for_call`` answers for the HALO3X3 packs."""
    rows = _replayed()
    assert len(rows) > 300 and sum(row[1] for row, _ in rows) > 5000
    wrong = [(row, G.table_row(row[0], pairs)) for row, pairs in rows if G.table_row(row[0], pairs) != row]
    assert not wrong, f"{len(wrong)} of {len(rows)} shapes differ, the first (recorded, now): {wrong[0]}"


def test_plan_is_the_single_source_of_layout_and_geometry():
    """``conv_pack_plan`` on plain integers gives the layout, k_pad, cout_pad and image size of every convolution pack of the table that
    was not refused, dense and grouped (the size in bytes: a split-float16 image is carried as float16 pairs, a grouped one as fp32)."""
    esize = {"float32": 4, "bfloat16": 2, "float16": 2, "float8_e4m3fn": 1}
    n = 0
    for spec, got in (pair for _, pairs in _replayed() for pair in pairs):
        if spec[0] != "conv" or got[0] == "raises":
            continue
        _, cout, cin, k, stride, pad, groups, dt, halo, act, f32, cin_pad, toggles, _ = spec
        dtype = G.DTYPES[dt]
        cin = max(cin, cin_pad or 0)
        if dtype == H.F16X2 and groups == 1:
            cin = -(-cin // 8) * 8
        hreg, flatk = H.HREG_128[0], H.FLAT_K_3X3[0]
        H.HREG_128[0], H.FLAT_K_3X3[0] = hreg and toggles != "hreg0", flatk and toggles != "flatk0"
        try:
            plan = H.conv_pack_plan(cout, cin, k, stride, pad, groups, H._act_code(bool(act)), dtype, None if halo is None else bool(halo), bool(f32))
        finally:
            H.HREG_128[0], H.FLAT_K_3X3[0] = hreg, flatk
        layout, k_pad, cout_pad, w_cin, _, shape, wdtype = got[:7]
        numel = 1
        for s in shape:
            numel *= s
        assert (plan.layout, plan.k_pad, plan.cout_pad, plan.cin) == (layout, k_pad, cout_pad, w_cin), spec
        assert plan.n_elems * H._ESIZE[dtype] == numel * esize[wdtype], spec
        n += 1
    assert n > 3000
