"""dy_stem2_fused in its dispatched form (8 x 16 tile, phase-B addresses from a table, hand-pipelined phases): the parent's bits, the tile
geometry against the CPU restatement, and the persistent tile walk.

The kernel's tile is TH x 16 layer-1 pixels (csrc/stem2_fused.hip, ``kS2FormTH``) and its grid at most 2 x 256 workgroups; the
shapes below are chosen around those two numbers.
"""
import importlib.util
import os

import pytest
import torch
import torch.nn.functional as F

from drone_yolo_amd import hip_ops as H
from tests._util import ROOT, golden, quantize

_spec = importlib.util.spec_from_file_location("make_stem2_golden", os.path.join(ROOT, "tools", "make_stem2_golden.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)
CASES, DTYPES, key, run_bits, stem2_case = G.CASES, G.DTYPES, G.key, G.run_bits, G.stem2_case

pytestmark = pytest.mark.gpu

TH, TW, GRID = 8, 16, 2 * 256
RTOL = {torch.bfloat16: 6e-3, torch.float16: 1.2e-3}  # one output rounding + accumulation order, as tests/test_kernels_gpu.py
DT = pytest.mark.parametrize("tag", list(DTYPES), ids=list(DTYPES))


@DT
@pytest.mark.parametrize("shape", CASES, ids=["2x36x44", "1x132x68"])
def test_stem2_parent_bits(shape, tag, device):
    """Every output bit is the one the 8 x 16 kernel of the parent commit wrote (tools/make_stem2_golden.py, recorded on the GPU)."""
    want = torch.from_numpy(golden("stem2_parent.npz")[key(shape, tag)].view("int16"))
    got = torch.from_numpy(run_bits(H, shape, DTYPES[tag], device).view("int16"))
    assert got.shape == want.shape
    assert torch.equal(got, want), f"{int((got != want).sum())} of {got.numel()} outputs differ from the parent's"


GEOMETRY = [
    ((2, 4 * (2 * TH + 1), 4 * 11), "H/4 = 2 TH + 1, W/4 = 11"),
    ((1, 4 * (3 * TH + 1), 4 * 25), "three tile rows + a ragged one, W/4 = 25"),
    ((3, 4, 4), "4x4"),
    ((1, 4 * TH, 4 * TW), "one exact tile"),
    ((1, 4 * (TH + 1), 4 * 2 * TW), "one row of tiles + one ragged row"),
    ((2, 4 * 2 * TH, 4 * 3 * TW), "exact tiles with an interior one"),
]


@DT
@pytest.mark.parametrize("shape", [g[0] for g in GEOMETRY], ids=[g[1] for g in GEOMETRY])
def test_stem2_tile_geometry(shape, tag, device):
    """Against the two F.conv2d with the kernel's rounding points; the channels of a wider buffer around the output stay untouched."""
    dtype = DTYPES[tag]
    n, h, w = shape
    img, w0, b0, w1, b1 = stem2_case(shape, dtype)
    ps = H.PackedStem2(w0, b0, True, w1, b1, True, dtype, device)
    out = torch.full((n, h // 4, w // 4, 80), 3.0, dtype=dtype, device=device).permute(0, 3, 1, 2)
    y = H.stem2_fused(img.to(device), ps, out=out[:, 8:72])
    torch.cuda.synchronize()
    mid = quantize(F.silu(F.conv2d(quantize(img, dtype), w0, b0, 2, 1)), dtype)
    ref = F.silu(F.conv2d(mid, w1, b1, 2, 1))
    got = y.float().cpu()
    assert tuple(got.shape) == tuple(ref.shape)
    scale = max(float(ref.abs().max()), 1e-6)
    err = float((got - ref).abs().max())
    assert err <= RTOL[dtype] * 1.5 * scale, f"stem2 {shape}: max|err| {err:.4e} vs scale {scale:.3f}"
    assert float((out[:, :8].float() - 3.0).abs().max()) == 0.0 and float((out[:, 72:].float() - 3.0).abs().max()) == 0.0


@DT
def test_stem2_tile_walk(tag, device):
    """A batch of at least three times the grid's tiles: workgroups walk several tiles (patch prefetch under the previous tile, epilogue scratch
    over the stem buffer).  An image's output does not depend on its batch position, nor on the batch around it."""
    dtype = DTYPES[tag]
    side = 256
    per_image = (side // 4 // TH) * (side // 4 // TW)
    n = -(-3 * GRID // per_image)
    assert n * per_image >= 3 * GRID
    g = torch.Generator().manual_seed(20)
    img = torch.rand(n, 3, side, side, generator=g)
    a, b = 1, n - 2
    img[b] = img[a]
    _, w0, b0, w1, b1 = stem2_case((1, side, side), dtype)
    ps = H.PackedStem2(w0, b0, True, w1, b1, True, dtype, device)
    y = H.stem2_fused(img.to(device), ps)
    alone = H.stem2_fused(img[a : a + 1].contiguous().to(device), ps)
    last = H.stem2_fused(img[n - 1 :].contiguous().to(device), ps)
    torch.cuda.synchronize()
    assert torch.equal(y[a], alone[0]), "image 1 of the batch differs from the same image run alone"
    assert torch.equal(y[a], y[b]), "the same image at two batch positions gives two results"
    assert torch.equal(y[n - 1], last[0]), "the batch's last image differs from the same image run alone"
