"""GPU: ``dy_process_mask`` over the geometry sweep of tests/_mask_util.py::PM_CASES against the float64 reference evaluated at run time
(tests/test_mask_geometry_host.py shows on the CPU that every case is sound and that the bar catches a moved crop edge, a missing half-pixel
offset, an unclamped corner, a cleared head and a bounding region one row too tight), and ``dy_mask_gather`` / ``dy_depth_to_space2_nhwc`` at
the borders their first tests left out.

The bar: no pixel of the whole masks differs from the reference outside the unsure set (|v| < 64 * 2^-23 * S, the golden fixtures' set), and
no byte outside the output is written: the masks are assembled into a slice of a buffer of 0xA5 bytes with guard bytes on both sides.
"""
import numpy as np
import pytest
import torch

from drone_yolo_amd import hip_ops as H
from tests._mask_util import NM, PM_TAGS, case_reference, check_masks
from tests.test_seg_gpu import _report

pytestmark = pytest.mark.gpu
GUARD = 72  # bytes on each side of the output: 8-byte aligned, not 16-byte


def _device_inputs(inp, device):
    """protos view, side, rows, count as tests/test_seg_gpu.py::test_process_mask_cases builds them; rows beyond the counts are NaN."""
    boxes, coef = torch.from_numpy(inp["boxes"]), inp["coef"]
    n, md = coef.shape[:2]
    side = torch.cat([boxes, coef], 2)
    rows = torch.cat([boxes, torch.zeros(n, md, 2)], 2)
    for b, k in enumerate(inp["counts"]):
        side[b, k:] = float("nan")
        rows[b, k:] = float("nan")
    count = torch.tensor(inp["counts"], dtype=torch.int32, device=device)
    return inp["protos"].to(device).permute(0, 3, 1, 2), side.to(device).contiguous(), rows.to(device).contiguous(), count


def _run(inp, dev_in, count=None):
    pv, side, rows, cnt = dev_in
    T, (oh, ow) = sum(inp["counts"]), inp["out_hw"]
    buf = torch.full((GUARD + T * oh * ow + GUARD,), 0xA5, dtype=torch.uint8, device=pv.device)
    out = buf[GUARD : GUARD + T * oh * ow]
    assert out.data_ptr() % 8 == 0
    kw = dict(ratio=inp["ratio"]) if inp["mode"] == "default" else dict(windows=inp["windows"], crop_rows=rows)
    got = H.process_mask(pv, side, cnt if count is None else count, inp["counts"], (oh, ow), out=out, **kw)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (T, oh, ow) and got.dtype == torch.uint8
    return got, buf


@pytest.mark.parametrize("tag", PM_TAGS)
def test_process_mask_geometry(tag, device):
    inp, (ref, unsure, inbox) = case_reference(tag)
    got, buf = _run(inp, _device_inputs(inp, device))
    host = buf.cpu().numpy()
    g = got.cpu().numpy()
    res = check_masks(g, ref, unsure, inbox)
    _report(f"process_mask geometry {tag}", {"masks": int(ref.shape[0]), "pixels": int(ref.size), **res})
    per_mask = ((g.astype(bool) != ref) & ~unsure).reshape(ref.shape[0], -1).sum(1)
    assert res["wrong"] == 0, f"{tag}: {res['wrong']} pixels differ from the float64 reference outside the unsure set, per mask {per_mask.tolist()}"
    assert (host[:GUARD] == 0xA5).all() and (host[-GUARD:] == 0xA5).all(), f"{tag}: bytes outside the output were written"
    assert int(g.max()) <= 1


def test_bad_out_is_refused_and_nothing_is_written(device):
    """On the device too, each defect alone is refused before a launch: the buffer keeps its fill."""
    inp, _ = case_reference("D1")
    pv, side, rows, cnt = _device_inputs(inp, device)
    T, (oh, ow) = sum(inp["counts"]), inp["out_hw"]
    n_out = T * oh * ow
    buf = torch.full((GUARD + 2 * n_out + GUARD,), 0xA5, dtype=torch.uint8, device=device)
    good = buf[GUARD : GUARD + n_out]
    assert good.data_ptr() % 8 == 0
    for bad, word in ((buf[GUARD + 4 : GUARD + 4 + n_out], "aligned"), (good[:-1], "elements"), (good.view(torch.int8), "dtype"),
                      (buf[GUARD : GUARD + 2 * n_out : 2], "contiguous"), (torch.zeros(n_out, dtype=torch.uint8), "device")):
        with pytest.raises(ValueError, match=f"out must be .*: .*{word}"):
            H.process_mask(pv, side, cnt, inp["counts"], (oh, ow), ratio=inp["ratio"], out=bad)
    torch.cuda.synchronize()
    assert bool((buf == 0xA5).all())


def test_device_count_below_host_count_gives_zero_masks(device):
    """A streamed run can see device counts of another batch than the host's: a row at or beyond the device count gives a zero mask."""
    inp, _ = case_reference("D1")
    assert inp["counts"] == [4, 8]
    dev_in = _device_inputs(inp, device)
    plain, _ = _run(inp, dev_in)
    fewer, buf = _run(inp, dev_in, count=torch.tensor([2, 8], dtype=torch.int32, device=device))
    assert not fewer[2:4].any() and plain[2:4].any()
    assert torch.equal(fewer[:2], plain[:2]) and torch.equal(fewer[4:], plain[4:])
    host = buf.cpu().numpy()
    assert (host[:GUARD] == 0xA5).all() and (host[-GUARD:] == 0xA5).all()


def test_two_launch_orders_are_identical(device):
    """Head and tail bytes are written by another workgroup than the aligned group next to them: a store to a byte that another workgroup
    owns would make two runs differ (one comparison, not a loop)."""
    inp, _ = case_reference("R8")
    dev_in = _device_inputs(inp, device)
    a, _ = _run(inp, dev_in)
    b, _ = _run(inp, dev_in)
    assert torch.equal(a, b)


def test_mask_gather_level_borders_and_bad_indices(device):
    hw, pitch, nc, md = [(6, 10), (3, 5), (2, 2), (1, 1)], [32, 36, 32, 40], 3, 8
    A = sum(h * w for h, w in hw)
    assert A == 80
    gen = torch.Generator().manual_seed(11)
    pred = torch.randn(2, 4 + nc + NM, A, generator=gen).to(device).contiguous()
    bufs = H.NmsBuffers(2, A, md, device)
    bufs.out.copy_(torch.randn(2, md, 6, generator=gen))
    bufs.count.copy_(torch.tensor([8, 4], dtype=torch.int32))
    index = torch.full((2, md), 7, dtype=torch.int32)
    index[0] = torch.tensor([0, 59, 60, 74, 75, 78, 79, 30])  # the first and last anchor of every level
    index[1, :4] = torch.tensor([-1, 80, 1000000, 5])
    bufs.index.copy_(index)
    levels, a0 = [], 0
    for (h, w), ld in zip(hw, pitch):
        buf = H.alloc_nhwc(2, ld, h, w, torch.float32, device)
        buf.fill_(float("nan"))  # the pad channels of a pitch above 32 are never read
        lv = buf[:, :NM]
        assert H.view_params(lv)[1] == ld
        lv.copy_(pred[:, 4 + nc :, a0 : a0 + h * w].reshape(2, NM, h, w))
        levels.append(lv)
        a0 += h * w
    sentinel = torch.full((2, md, 4 + NM), -7.0, device=device)
    a = H.mask_gather(bufs, pred=pred, nc=nc, out=sentinel.clone())
    b = H.mask_gather(bufs, levels=levels, out=sentinel.clone())
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    exp = sentinel.clone()
    for i, k in enumerate([8, 4]):
        idx = index[i, :k].long()
        ok = (idx >= 0) & (idx < A)
        exp[i, :k, :4] = bufs.out[i, :k, :4]
        exp[i, :k, 4:] = 0.0
        exp[i, :k][ok.to(device), 4:] = pred[i, 4 + nc :, idx[ok].to(device)].T
    assert torch.equal(a, exp)
    assert bool((a[1, :3, 4:] == 0).all()) and torch.equal(a[1, :3, :4], bufs.out[1, :3, :4])  # bad index: zero coefficients, the box copied
    assert bool((a[1, 3, 4:] != 0).any())
    assert bool((a[1, 4:] == -7.0).all())  # rows beyond the count keep their sentinel


@pytest.mark.parametrize("shape", [(1, 8, 1, 1), (2, 8, 1, 9), (1, 64, 33, 31)], ids=["1x1", "1x9", "33x31"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32], ids=["f16", "bf16", "f32"])
def test_depth_to_space_small_and_wide(dtype, shape, device):
    n, c, h, w = shape
    buf = H.alloc_nhwc(n, 4 * c + 16, h, w, dtype, device)  # source and destination: channel slices of wider buffers
    buf.copy_(torch.randn(buf.shape, device=device).to(dtype))
    x = buf[:, 8 : 8 + 4 * c]
    wide = H.alloc_nhwc(n, c + 8, 2 * h, 2 * w, dtype, device)
    wide.fill_(-3.0)
    y = H.depth_to_space2(x, out=wide[:, :c])
    torch.cuda.synchronize()
    ref = x.reshape(n, 2, 2, c, h, w).permute(0, 3, 4, 1, 5, 2).reshape(n, c, 2 * h, 2 * w)
    assert torch.equal(y, ref)
    assert bool((wide[:, c:] == -3.0).all())  # the destination's other channels are not written
