"""The register-weight 3x3 family (conv3x3_hreg, conv3x3_hreg_s2, conv3x3_hhead) on the shapes at which its item pipeline can go wrong, and
the Detect-branch tail of conv3x3_hhead, which no longer waits for vector memory inside a tile (stores through buffer descriptors, the
candidate list finished one tile late from scalar state).

Convolutions: fp32 CPU convolution on dtype-rounded inputs, tolerance of tests/test_kernels_gpu.py (RTOL x scale).  Shapes: one tile
(the pipeline's prologue is its epilogue), four tiles with one-pixel ragged edges, odd maps over several images, and 2,400 tiles over
at most 768 workgroups (three or four tiles per workgroup, uneven remainder).  cin 32 stays on conv3x3_halo (dy_conv3x3_halo_route), which
the case asserts.  Detect branches: scores / boxes against the fp32 CPU chain with the bounds of
test_detect_branch_fused_matches_cpu_chain; the candidate list must be exactly the set that follows from the kernel's own scores.
Repeatability: five runs beside another convolution on a second stream, bit-identical (stale halo reads were this family's failure)."""
import zlib

import pytest
import torch
import torch.nn.functional as F

from drone_yolo_amd import hip_ops as H
from oracle import drone_yolo_oracle as O
from tests._util import quantize

pytestmark = pytest.mark.gpu

RTOL = {torch.bfloat16: 6e-3, torch.float16: 1.2e-3}  # tests/test_kernels_gpu.py
DT = [torch.bfloat16, torch.float16]
DT_IDS = ["bf16", "f16"]


def nhwc(t, dtype, dev):
    return t.permute(0, 2, 3, 1).contiguous().to(dtype).to(dev).permute(0, 3, 1, 2)


def back(t):
    return t.float().cpu().contiguous()


def check_close(got, ref, dtype, what):
    scale = max(float(ref.abs().max()), 1e-6)
    err = float((got - ref).abs().max())
    assert err <= RTOL[dtype] * scale, f"{what}: max|err| {err:.4e} vs scale {scale:.3f} (tol {RTOL[dtype] * scale:.4e})"


def conv_case(cin, cout, stride, b, h, w, act, dtype, device):
    g = torch.Generator().manual_seed(zlib.crc32(f"{cin}-{cout}-{stride}-{b}-{h}-{w}-{act}".encode()) % 1000)
    x = quantize(torch.randn(b, cin, h, w, generator=g), dtype)
    wt = quantize(torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (cin * 9)) ** 0.5, dtype)
    bias = torch.randn(cout, generator=g) * 0.2
    ref = F.conv2d(x, wt, bias, stride, 1)
    ref = F.silu(ref) if act else ref
    pc = H.PackedConv(wt, bias, stride, 1, 1, act, dtype, device)
    return x, pc, ref


def expected_kernel(cin, stride, act, dtype):
    if stride == 2:
        return "conv3x3_hreg_s2"
    if cin == 32:
        return "conv3x3_halo"  # one chunk per tile measured no gain on the register-weight kernel: dy_conv3x3_halo_route declines it
    if cin == 128 and act and dtype == torch.bfloat16:
        return None  # bf16 inference packs of 128 channels stay on the virtual-flat GEMM (hip_ops.PackedConv)
    return "conv3x3_hreg_kernel"


S1_SHAPES = [(1, 8, 16), (1, 9, 17), (3, 33, 31)]


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("act", [True, False], ids=["silu", "noact"])
@pytest.mark.parametrize("cout", [64, 128])
@pytest.mark.parametrize("cin", [32, 64, 128])
def test_stride1_matches_cpu(cin, cout, act, dtype, device):
    for b, h, w in S1_SHAPES:
        x, pc, ref = conv_case(cin, cout, 1, b, h, w, act, dtype, device)
        y = H.conv2d(nhwc(x, dtype, device), pc)
        torch.cuda.synchronize()
        want = expected_kernel(cin, 1, act, dtype)
        if want is not None:
            assert H.last_kernel_name().startswith(want), (H.last_kernel_name(), want)
        check_close(back(y), ref, dtype, f"3x3 s1 {cin}->{cout} {b}x{h}x{w} act={act}")


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("act", [True, False], ids=["silu", "noact"])
def test_stride1_many_tiles_per_workgroup(act, dtype, device):
    """80 x 80, B = 48: 2,400 tiles over at most 768 workgroups."""
    x, pc, ref = conv_case(64, 64, 1, 48, 80, 80, act, dtype, device)
    y = H.conv2d(nhwc(x, dtype, device), pc)
    torch.cuda.synchronize()
    assert H.last_kernel_name().startswith("conv3x3_hreg_kernel"), H.last_kernel_name()
    check_close(back(y), ref, dtype, f"3x3 s1 64->64 48x80x80 act={act}")


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("act", [True, False], ids=["silu", "noact"])
@pytest.mark.parametrize("cout", [64, 128])
def test_stride2_matches_cpu(cout, act, dtype, device):
    for b, h, w in [(1, 8, 8), (3, 33, 31), (2, 160, 160)]:
        x, pc, ref = conv_case(64, cout, 2, b, h, w, act, dtype, device)
        y = H.conv2d(nhwc(x, dtype, device), pc)
        torch.cuda.synchronize()
        assert H.last_kernel_name().startswith("conv3x3_hreg_s2"), H.last_kernel_name()
        check_close(back(y), ref, dtype, f"3x3 s2 64->{cout} {b}x{h}x{w} act={act}")


# ---- Detect branches ----
def branch_case(nc, b, h, w, dtype, device):
    """One level of a legacy-v8 Detect head from the branches' first conv outputs on: operands, CPU reference, packed device operands."""
    g = torch.Generator().manual_seed(zlib.crc32(f"branch-{nc}-{b}-{h}-{w}".encode()) % 1000)
    q = lambda t: quantize(t, dtype)  # noqa: E731
    xs = [q(torch.randn(b, 64, h, w, generator=g)) for _ in range(2)]
    w3 = [q(torch.randn(64, 64, 3, 3, generator=g) * (2.0 / (64 * 9)) ** 0.5) for _ in range(2)]
    b3 = [torch.randn(64, generator=g) * 0.2 for _ in range(2)]
    w1 = [q(torch.randn(co, 64, 1, 1, generator=g) * 0.15) for co in (64, nc)]
    b1 = [torch.randn(co, generator=g) * 0.3 for co in (64, nc)]
    stride = 4.0
    with torch.no_grad():
        mids = [q(F.silu(F.conv2d(xs[k], w3[k], b3[k], 1, 1))) for k in range(2)]  # the trunk activation's rounding point
        feats = torch.cat([F.conv2d(mids[k].double(), w1[k].double(), b1[k].double()).float() for k in range(2)], 1)
        ref = O.detect_decode([feats], [stride], nc)
    dev = dict(x=[nhwc(t, dtype, device) for t in xs], pc3=[H.PackedConv(w3[k], b3[k], 1, 1, 1, True, dtype, device) for k in range(2)],
               w1=[H.pack_frag1x1(w1[k], b1[k], dtype, device) for k in range(2)], stride=stride)
    return dev, ref


def run_branches(dev, nc, b, h, w, device, conf, mask=None):
    A = h * w
    pred = torch.zeros((b, 4 + nc, A), dtype=torch.float32, device=device)
    bufs = H.NmsBuffers(b, A, 300, device)
    bufs.workspace.zero_()
    H.nms_reset_counts(bufs)
    H.detect_branch_fused(dev["x"][0], dev["pc3"][0], dev["w1"][0][0], dev["w1"][0][1], 1, nc, 16, dev["stride"], pred, 0)
    assert H.last_kernel_name().startswith("conv3x3_hhead"), H.last_kernel_name()
    H.detect_branch_fused(dev["x"][1], dev["pc3"][1], dev["w1"][1][0], dev["w1"][1][1], 2, nc, 16, dev["stride"], pred, 0, nms_bufs=bufs, conf_thres=conf,
                          classes_mask=mask)
    assert H.last_kernel_name().startswith("conv3x3_hhead"), H.last_kernel_name()
    torch.cuda.synchronize()
    return pred, bufs


def candidates(bufs, b, A):
    """(counts, per-image sorted key lists, cls table) out of the dy_nms workspace (csrc/nms_ws.h)."""
    ws = bufs.workspace.cpu()
    P = 1
    while P < A:
        P <<= 1
    off_keys = (b * 4 + 255) // 256 * 256
    counts = ws[: b * 4].view(torch.int32).tolist()
    keys = ws[off_keys : off_keys + b * P * 8].view(torch.int64).reshape(b, P)
    cls = ws[off_keys + b * P * 8 : off_keys + b * P * 8 + b * A * 2].view(torch.int16).reshape(b, A)
    return counts, keys, cls


BRANCH_SHAPES = [(1, 8, 16), (2, 20, 20), (3, 33, 31)]


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("nc", [1, 10, 16])
def test_detect_branches_match_cpu_chain_and_list_their_own_candidates(nc, dtype, device):
    for b, h, w in BRANCH_SHAPES:
        dev, ref = branch_case(nc, b, h, w, dtype, device)
        A = h * w
        # conf 0: every anchor of every tile is a candidate; 1.0: a sigmoid never exceeds it, no tile has one; 0.5: some
        for conf in (0.0, 1.0, 0.5):
            pred, bufs = run_branches(dev, nc, b, h, w, device, conf)
            y = pred.cpu()
            assert bool(torch.isfinite(y).all())
            box_tol = (0.03 if dtype == torch.bfloat16 else 0.004) * float(ref[:, :4].abs().max())
            cls_tol = 0.03 if dtype == torch.bfloat16 else 0.004
            what = f"nc {nc} {b}x{h}x{w} conf {conf}"
            assert float((y[:, :4] - ref[:, :4]).abs().max()) <= box_tol, (what, float((y[:, :4] - ref[:, :4]).abs().max()), box_tol)
            assert float((y[:, 4:] - ref[:, 4:]).abs().max()) <= cls_tol, (what, float((y[:, 4:] - ref[:, 4:]).abs().max()))
            counts, keys, cls = candidates(bufs, b, A)
            best, bj = y[:, 4:].max(1)  # (first maximum, as cls.max(1))
            for n in range(b):
                hit = torch.nonzero(best[n] > conf).flatten()
                bits = best[n][hit].view(torch.int32).to(torch.int64) & 0xFFFFFFFF
                want = ((~bits & 0xFFFFFFFF) << 32) | hit  # (the u64 key read as int64: the shift wraps the same way)
                got = keys[n, : counts[n]]
                assert counts[n] == hit.numel(), (what, n, counts[n], hit.numel())
                assert torch.equal(torch.sort(got).values, torch.sort(want).values), (what, n)
                listed = cls[n][hit].to(torch.int64)  # the listed class holds the best score (an exact tie may name either index on the CPU)
                assert bool((listed < nc).all()) and torch.equal(y[n, 4:][listed, hit], best[n][hit]), (what, n)


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
def test_class_mask_drops_masked_classes_from_the_candidates(dtype, device):
    nc, b, h, w = 10, 2, 20, 20
    dev, _ = branch_case(nc, b, h, w, dtype, device)
    mask = torch.ones(nc, dtype=torch.uint8)
    mask[[0, 3, 7]] = 0
    pred, bufs = run_branches(dev, nc, b, h, w, device, 0.3, mask=mask.to(device))
    counts, keys, cls = candidates(bufs, b, h * w)
    best, bj = pred.cpu()[:, 4:].max(1)
    for n in range(b):
        hit = torch.nonzero((best[n] > 0.3) & (mask[bj[n]] != 0)).flatten()
        assert counts[n] == hit.numel(), (n, counts[n], hit.numel())
        assert torch.equal(torch.sort(keys[n, : counts[n]] & 0xFFFFFFFF).values, hit), n
        assert torch.equal(pred.cpu()[n, 4:][cls[n][hit].to(torch.int64), hit], best[n][hit]), n


# ---- repeatability beside another stream's kernels ----
@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
def test_five_runs_beside_another_stream_are_bit_identical(dtype, device):
    x, pc, ref = conv_case(64, 128, 1, 6, 80, 80, True, dtype, device)
    xo, pco, _ = conv_case(64, 64, 1, 8, 80, 80, True, dtype, device)
    xd, xod = nhwc(x, dtype, device), nhwc(xo, dtype, device)
    nc, b, h, w = 10, 4, 40, 40
    dev, _ = branch_case(nc, b, h, w, dtype, device)
    side = torch.cuda.Stream(device=device)
    torch.cuda.synchronize()
    outs, preds, lists = [], [], []
    for _ in range(5):
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            for _ in range(4):
                H.conv2d(xod, pco)
        y = H.conv2d(xd, pc)
        assert H.last_kernel_name().startswith("conv3x3_hreg_kernel"), H.last_kernel_name()
        with torch.cuda.stream(side):
            for _ in range(4):
                H.conv2d(xod, pco)
        pred, bufs = run_branches(dev, nc, b, h, w, device, 0.4)
        torch.cuda.synchronize()
        counts, keys, cls = candidates(bufs, b, h * w)
        outs.append(y.cpu().clone())
        preds.append(pred.cpu().clone())
        lists.append((counts, [torch.sort(keys[n, : counts[n]]).values for n in range(b)]))
    check_close(back(outs[0]), ref, dtype, "3x3 s1 64->128 6x80x80")
    for k in range(1, 5):
        assert torch.equal(outs[k].view(torch.int16), outs[0].view(torch.int16)), f"conv run {k} differs from run 0"
        assert torch.equal(preds[k].view(torch.int32), preds[0].view(torch.int32)), f"branch run {k} differs from run 0"
        assert lists[k][0] == lists[0][0] and all(torch.equal(a, c) for a, c in zip(lists[k][1], lists[0][1])), f"candidates of run {k} differ"
