"""The three Detect decode kernels (detect_decode_kernel, detect_head_kernel for f32 / bf16 / f16, detect_head_split_kernel) share one
decode row and one candidate append (csrc/detect_row.h).  Every case here is compared with what the kernels of the commit before that
header wrote, bit for bit: tests/golden/detect_rows_parent.npz, recorded on the GPU by tools/make_detect_rows_golden.py, which also
builds the inputs (fixed seeds) and documents the file.  The decoded tensor must be equal; of the candidate filter the counts, each
image's keys (sorted: the append order is not deterministic) and the class stored for each surviving anchor.

The shapes are the smallest at which the code can go wrong: a level of 575 anchors (nine 64-anchor tiles, the last ragged, two
workgroup groups in the head kernel), one of fewer than 64 anchors and one of a single anchor; nc 10 with a class mask, once nc 1.
The inputs and the oracle's view of them need no GPU: ``test_conf_keeps_some_candidates_and_rejects_some`` runs on the CPU.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

from drone_yolo_amd import hip_ops as H
from tests._util import ROOT, golden

_spec = importlib.util.spec_from_file_location("make_detect_rows_golden", os.path.join(ROOT, "tools", "make_detect_rows_golden.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

IDS = [G.case_name(k, nc) for k, nc in G.CASES]


@pytest.mark.parametrize("kernel,nc", G.CASES, ids=IDS)
def test_conf_keeps_some_candidates_and_rejects_some(kernel, nc):
    """By the oracle's decode and by the recorded counts: every image has candidates, anchors below conf, and (nc 10) anchors that
    only the class mask removes."""
    above, kept = G.oracle_candidates(kernel, nc)
    counts = golden("detect_rows_parent.npz")[f"{G.case_name(kernel, nc)}_counts"].tolist()
    print(f"{G.case_name(kernel, nc)}: oracle {above} above conf, {kept} behind the mask; recorded {counts} of {G.ANCHORS}")
    assert len(counts) == G.BATCH
    for a, k, c in zip(above, kept, counts):
        assert 0 < k < G.ANCHORS and 0 < c < G.ANCHORS
        assert k < a or nc == 1
        assert abs(c - k) <= 2  # the device rounds a score next to conf the other way at most here and there


@pytest.mark.gpu
@pytest.mark.parametrize("kernel,nc", G.CASES, ids=IDS)
def test_detect_rows_equal_parent_bits(kernel, nc, device):
    g = golden("detect_rows_parent.npz")
    name = G.case_name(kernel, nc)
    got = G.run_case(H, kernel, nc, device)
    want_pred = torch.from_numpy(G.unplanes(g[f"{name}_pred"], (G.BATCH, 4 + nc, G.ANCHORS)))
    assert torch.equal(torch.from_numpy(got["pred"]), want_pred), f"{name}: decoded tensor differs in {int((torch.from_numpy(got['pred']) != want_pred).sum())} values"
    assert np.array_equal(got["counts"], g[f"{name}_counts"]), f"{name}: counts {got['counts'].tolist()} vs {g[f'{name}_counts'].tolist()}"
    assert np.array_equal(got["keys"], g[f"{name}_keys"]), f"{name}: sorted keys differ"
    assert np.array_equal(got["cls"], g[f"{name}_cls"]), f"{name}: classes of the surviving anchors differ"
    assert all(0 < c < G.ANCHORS for c in got["counts"].tolist())
