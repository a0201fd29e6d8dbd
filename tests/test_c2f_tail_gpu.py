"""dy_c2f_tail_fused (csrc/conv3x3_hc2f.hip): the last Bottleneck's 3x3 and the closing 1x1 of a hidden-64 C2f block in one launch.

Op level: against the CPU chain q(silu(conv3x3)) [+ y_prev -> q] -> cat -> q(silu(conv1x1)) on dtype-rounded operands, bound
RTOL x 3 x max|ref| (test_c2f_fused_block_matches_cpu_chain_and_layerwise's).  The concat-buffer head is a view with pitch
(1 + n) * 64 + 16 at channel offset 8, the output a channel slice of a wider buffer whose neighbours must keep their sentinel.
The block-level cases also ask for bit-identity with the layer-by-layer path.
Shapes: one tile (the pipeline's prologue is its epilogue), four tiles with one-pixel ragged edges, odd maps over several images, and
2,400 tiles (several tiles per workgroup, uneven remainder).  Block level: C2f(128, 128) with fuse_block on against off.
Repeatability: five runs beside another convolution on a second stream, bit-identical (stale LDS reads were this family's failure)."""
import functools
import zlib

import pytest
import torch
import torch.nn.functional as F

from drone_yolo_amd import hip_ops as H
from tests._util import quantize

pytestmark = pytest.mark.gpu

RTOL = {torch.bfloat16: 6e-3, torch.float16: 1.2e-3}  # tests/test_kernels_gpu.py
DT = [torch.bfloat16, torch.float16]
DT_IDS = ["bf16", "f16"]
KERNEL = "conv3x3_hc2f"
C = 64  # hidden


def nhwc(t, dtype, dev, ld=None, c_off=0):
    n, c, h, w = t.shape
    ld = c if ld is None else ld
    buf = torch.zeros((n, h, w, ld), dtype=dtype, device=dev)
    buf[..., c_off : c_off + c] = t.permute(0, 2, 3, 1).to(dtype).to(dev)
    return buf.permute(0, 3, 1, 2)[:, c_off : c_off + c]


def back(t):
    return t.float().cpu().contiguous()


def check_close(got, ref, dtype, what, extra=3.0):
    scale = max(float(ref.abs().max()), 1e-6)
    err = float((got - ref).abs().max())
    print(f"{what}: max|err| {err:.4e}, bound {RTOL[dtype] * extra * scale:.4e}")
    assert err <= RTOL[dtype] * extra * scale, f"{what}: max|err| {err:.4e} vs scale {scale:.3f} (tol {RTOL[dtype] * extra * scale:.4e})"


@functools.lru_cache(maxsize=None)
def tail_case(n, shortcut, b, h, w, dtype):
    """Operands (dtype-rounded, CPU) and the CPU chain's result; built once per case and left unchanged."""
    g = torch.Generator().manual_seed(zlib.crc32(f"c2f-tail-{n}-{shortcut}-{b}-{h}-{w}".encode()) % 1000)
    q = lambda t: quantize(t, dtype)  # noqa: E731
    t = q(torch.randn(b, C, h, w, generator=g))
    ybuf = q(torch.randn(b, (1 + n) * C, h, w, generator=g))
    w3 = q(torch.randn(C, C, 3, 3, generator=g) * (2.0 / (C * 9)) ** 0.5)
    b3 = torch.randn(C, generator=g) * 0.2
    w1 = q(torch.randn(128, (2 + n) * C, 1, 1, generator=g) * (2.0 / ((2 + n) * C)) ** 0.5)
    b1 = torch.randn(128, generator=g) * 0.2
    with torch.no_grad():
        y_last = F.silu(F.conv2d(t, w3, b3, 1, 1))
        y_last = q(y_last + ybuf[:, n * C :]) if shortcut else q(y_last)
        ref = q(F.silu(F.conv2d(torch.cat((ybuf, y_last), 1), w1, b1)))
    return t, ybuf, (w3, b3), (w1, b1), ref


SENTINEL = 7.0


def run_tail(case, n, shortcut, dtype, device):
    t, ybuf, mcv2, cv2, _ = case
    b, _, h, w = t.shape
    pk = H.PackedC2fTail(mcv2, cv2, n=n, shortcut=shortcut, dtype=dtype, device=device)
    td = nhwc(t, dtype, device)
    yd = nhwc(ybuf, dtype, device, ld=(1 + n) * C + 16, c_off=8)
    wide = torch.full((b, h, w, 128 + 32), SENTINEL, dtype=dtype, device=device).permute(0, 3, 1, 2)
    out = H.c2f_tail_fused(td, yd, pk, out=wide[:, 16:144])
    return out, wide, (td, yd, pk)


FORMS = [(1, False), (2, True), (1, True), (2, False)]
FORM_IDS = ["n1", "n2-shortcut", "n1-shortcut", "n2"]
SHAPES = [(1, 8, 16), (1, 9, 17), (3, 33, 31), (12, 160, 160)]


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_tail_matches_cpu_chain(shape, form, dtype, device):
    n, shortcut = form
    assert H.c2f_tail_fused_supported(C, 128, n, dtype)
    case = tail_case(n, shortcut, *shape, dtype)
    out, wide, _ = run_tail(case, n, shortcut, dtype, device)
    torch.cuda.synchronize()
    assert H.last_kernel_name().startswith(KERNEL), H.last_kernel_name()
    check_close(back(out), case[4], dtype, f"c2f tail n={n} shortcut={shortcut} {shape}")
    # slice neighbours: the wider buffer's other channels keep their sentinel
    assert bool((wide[:, :16] == SENTINEL).all()) and bool((wide[:, 144:] == SENTINEL).all()), "the launch wrote outside its channel slice"


def make_block(n, shortcut, seed, c=128, wstd=0.08):
    from drone_yolo_amd.nn.modules import C2f

    g = torch.Generator().manual_seed(seed)
    blk = C2f(c, c, n=n, shortcut=shortcut).eval()
    for prm in blk.parameters():
        prm.data = torch.randn(prm.shape, generator=g) * (wstd if prm.dim() > 1 else 0.3) + (1.0 if prm.dim() == 1 else 0.0)
    for m in blk.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.1)
            m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)
            m.eps = 1e-3
    return blk, g


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("shape", [(2, 40, 36), (1, 33, 50)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("n,shortcut", [(1, False), (2, True)], ids=["n1", "n2-shortcut"])
def test_block_fused_tail_agrees_with_layer_by_layer(n, shortcut, shape, dtype, device):
    """C2f(128, 128): fuse_block on (the dispatched forms end in the fused launch) against off (the true layer-by-layer path)."""
    from drone_yolo_amd.nn.modules import C2f

    blk, g = make_block(n, shortcut, shape[1])
    b, h, w = shape
    x = quantize(torch.randn(b, 128, h, w, generator=g), dtype)
    blk = blk.to(device)
    xd = nhwc(x, dtype, device, ld=128 + 16, c_off=8)
    blk.fuse_block = True
    got = blk(xd)
    torch.cuda.synchronize()
    assert (n, shortcut) in C2f.fuse_tail_forms  # both forms of Drone-YOLO-s are dispatched
    assert H.last_kernel_name().startswith(KERNEL), H.last_kernel_name()
    blk.fuse_block = False
    layerwise = blk(xd)
    torch.cuda.synchronize()
    assert H.last_kernel_name().startswith("conv1x1_stream"), H.last_kernel_name()
    check_close(back(got), back(layerwise), dtype, f"C2f(128, 128, n={n}, shortcut={shortcut}) {shape}: fuse_block on vs off")
    # the fused launch sums as its two launches do (3x3: chunks, taps in order from the bias; 1x1: K ascending from zero, bias last)
    assert torch.equal(got.contiguous().view(torch.int16), layerwise.contiguous().view(torch.int16)), "fused tail is not bit-identical to the layer-by-layer path"


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("form", [(1, False), (2, True)], ids=["n1", "n2-shortcut"])
def test_five_runs_beside_another_stream_are_bit_identical(form, dtype, device):
    n, shortcut = form
    case = tail_case(n, shortcut, 3, 33, 31, dtype)
    g = torch.Generator().manual_seed(5)
    xo = nhwc(quantize(torch.randn(8, 64, 80, 80, generator=g), dtype), dtype, device)
    pco = H.PackedConv(quantize(torch.randn(64, 64, 3, 3, generator=g) * 0.05, dtype), torch.zeros(64), 1, 1, 1, True, dtype, device)
    side = torch.cuda.Stream(device=device)
    torch.cuda.synchronize()
    outs = []
    for _ in range(5):
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            for _ in range(4):
                H.conv2d(xo, pco)
        out, _, keep = run_tail(case, n, shortcut, dtype, device)
        assert H.last_kernel_name().startswith(KERNEL), H.last_kernel_name()
        torch.cuda.synchronize()
        outs.append(out.cpu().clone())
    check_close(back(outs[0]), case[4], dtype, f"c2f tail n={n} shortcut={shortcut} 3x33x31 beside a second stream")
    for k in range(1, 5):
        assert torch.equal(outs[k].view(torch.int16), outs[0].view(torch.int16)), f"run {k} differs from run 0"


@pytest.mark.parametrize("c,shortcut,shape,kernel", [(64, True, (3, 16, 16), "c2f_fused_kernel"), (128, False, (2, 40, 36), KERNEL)], ids=["block-64", "tail-128"])
def test_fused_packs_follow_a_training_phase_of_the_block_alone(c, shortcut, shape, kernel, device):
    """A C2f used on its own: an eval pass fills the fused slot (dy_c2f_fused at 64 channels, dy_c2f_tail_fused at 128), one training-mode
    forward moves the BatchNorm running statistics through raw pointers (torch's version counters see nothing), and back in eval mode the
    fused launch must run on the NEW statistics, as the layer-by-layer path does: the block's own train() drops its packs.  float16, the
    smallest shapes of test_c2f_fused_block_matches_cpu_chain_and_layerwise / test_block_fused_tail_agrees_with_layer_by_layer, their bound."""
    dtype = torch.float16
    blk, g = make_block(1, shortcut, shape[1], c=c, wstd=0.12 if c == 64 else 0.08)
    b, h, w = shape
    x = quantize(torch.randn(b, c, h, w, generator=g) + 1.0, dtype)  # per-channel mean well away from the running means (~ 0.1)
    blk = blk.to(device)
    xd = nhwc(x, dtype, device)
    blk.fuse_block = True
    blk(xd)
    assert H.last_kernel_name().startswith(kernel), H.last_kernel_name()
    bns = [blk.cv1.bn, blk.m[0].cv1.bn, blk.m[0].cv2.bn, blk.cv2.bn]
    start = [bn.running_mean.clone() for bn in bns]
    blk.train()
    blk(xd)
    blk.eval()
    torch.cuda.synchronize()
    for bn, m0 in zip(bns, start):
        assert not torch.equal(bn.running_mean, m0), "the training forward left a running mean where it was"
    got = blk(xd)
    torch.cuda.synchronize()
    assert H.last_kernel_name().startswith(kernel), H.last_kernel_name()
    blk.fuse_block = False
    layerwise = blk(xd)
    torch.cuda.synchronize()
    check_close(back(got), back(layerwise), dtype, f"C2f({c}, {c}, n=1, shortcut={shortcut}) {shape} after train() / eval(): fuse_block on vs off", extra=3.0)
