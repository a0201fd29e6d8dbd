"""dy_c2f_front_fused (csrc/conv3x3_hdown.hip): the stride-2 3x3 in front of a hidden-64 C2f block and the block's opening 1x1 in one launch.

Op level: against the CPU chain q(silu(conv3x3 s2)) -> [cat other] -> q(silu(conv1x1)) on dtype-rounded operands, bound RTOL x 3 x max|ref|
(tests/test_c2f_tail_gpu.py's).  Form A: 64 -> 128, no second source; form B: 64 -> 64 with 128 channels of a second Concat source, a view at
channel offset 8 with pitch 128 + 16.  The output is a channel slice of a wider buffer whose neighbours must keep their sentinel.
Input sizes: 8 x 32 (one output tile: the pipeline's prologue is its epilogue), 10 x 34 (5 x 17 outputs: four tiles with one-pixel ragged edges),
3 x 33 x 31 (odd sizes, Ho = (H - 1) / 2 + 1) and 8 x 160 x 160 (3,200 tiles: several per workgroup, uneven remainder).
Block level and whole model: bit-identity with the two-launch path.  Repeatability: five runs beside another convolution on a second stream,
bit-identical (stale LDS reads were this family's failure)."""
import functools
import zlib

import pytest
import torch
import torch.nn.functional as F

from drone_yolo_amd import hip_ops as H
from tests._util import load_yaml, quantize

pytestmark = pytest.mark.gpu

RTOL = {torch.bfloat16: 6e-3, torch.float16: 1.2e-3}  # tests/test_kernels_gpu.py
DT = [torch.bfloat16, torch.float16]
DT_IDS = ["bf16", "f16"]
KERNEL = "conv3x3_hdown"
ENTRY = "dy_c2f_front_fused"
FORMS = {"A": (128, 0), "B": (64, 128)}  # (cmid, c_other)
SENTINEL = 7.0


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
def front_case(form, b, h, w, dtype):
    """Operands (dtype-rounded, CPU) and the CPU chain's result; built once per case and left unchanged."""
    cmid, c_other = FORMS[form]
    g = torch.Generator().manual_seed(zlib.crc32(f"c2f-front-{form}-{b}-{h}-{w}".encode()) % 1000)
    q = lambda t: quantize(t, dtype)  # noqa: E731
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    x = q(torch.randn(b, 64, h, w, generator=g))
    other = q(torch.randn(b, c_other, ho, wo, generator=g)) if c_other else None
    w3 = q(torch.randn(cmid, 64, 3, 3, generator=g) * (2.0 / (64 * 9)) ** 0.5)
    b3 = torch.randn(cmid, generator=g) * 0.2
    w1 = q(torch.randn(128, cmid + c_other, 1, 1, generator=g) * (2.0 / (cmid + c_other)) ** 0.5)
    b1 = torch.randn(128, generator=g) * 0.2
    with torch.no_grad():
        mid = q(F.silu(F.conv2d(x, w3, b3, 2, 1)))
        ref = q(F.silu(F.conv2d(mid if other is None else torch.cat((mid, other), 1), w1, b1)))
    return x, other, (w3, b3), (w1, b1), ref


def run_front(case, dtype, device):
    x, other, conv3, cv1, ref = case
    b, _, ho, wo = ref.shape
    pk = H.PackedC2fFront(conv3, cv1, H.DY_ACT_SILU, dtype, device)
    xd = nhwc(x, dtype, device)
    od = None if other is None else nhwc(other, dtype, device, ld=128 + 16, c_off=8)
    wide = torch.full((b, ho, wo, 128 + 32), SENTINEL, dtype=dtype, device=device).permute(0, 3, 1, 2)
    out = H.c2f_front_fused(xd, pk, other=od, out=wide[:, 16:144])
    return out, wide, (xd, od, pk)


SHAPES = [(1, 8, 32), (1, 10, 34), (3, 33, 31), (8, 160, 160)]


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("form", ["A", "B"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_front_matches_cpu_chain(shape, form, dtype, device):
    cmid, c_other = FORMS[form]
    assert H.c2f_front_fused_supported(64, cmid, c_other, 128, dtype)
    case = front_case(form, *shape, dtype)
    out, wide, _ = run_front(case, dtype, device)
    torch.cuda.synchronize()
    assert H.last_kernel_name().startswith(KERNEL), H.last_kernel_name()
    check_close(back(out), case[4], dtype, f"c2f front form {form} {shape}")
    # slice neighbours: the wider buffer's other channels keep their sentinel
    assert bool((wide[:, :16] == SENTINEL).all()) and bool((wide[:, 144:] == SENTINEL).all()), "the launch wrote outside its channel slice"


def randomize(mod, g):
    for prm in mod.parameters():
        prm.data = torch.randn(prm.shape, generator=g) * (0.08 if prm.dim() > 1 else 0.3) + (1.0 if prm.dim() == 1 else 0.0)
    for m in mod.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.1)
            m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)
            m.eps = 1e-3
    return mod.eval()


def entries(plan):
    return [fn.__name__ for fn, _, _ in plan.ops]


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("shape", [(2, 24, 40), (1, 160, 160)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("form", ["A", "B"])
def test_block_fused_front_is_bit_identical_to_two_launches(form, shape, dtype, device):
    """A: [RepVGGBlock(64, 128, 3, 2) -> C2f(128, 128, n=2, shortcut=True)];  B: [Conv(64, 64, 3, 2), Concat, C2f(192, 128, n=1)]."""
    from drone_yolo_amd.nn.modules import C2f, Concat, Conv, RepVGGBlock

    g = torch.Generator().manual_seed(shape[1] + ord(form))
    b, h, w = shape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    if form == "A":
        prod, blk = randomize(RepVGGBlock(64, 128, 3, 2), g), randomize(C2f(128, 128, n=2, shortcut=True), g)
    else:
        prod, blk = randomize(Conv(64, 64, 3, 2), g), randomize(C2f(192, 128, n=1), g)
    prod, blk = prod.to(device), blk.to(device)
    xd = nhwc(quantize(torch.randn(b, 64, h, w, generator=g), dtype), dtype, device)
    od = nhwc(quantize(torch.randn(b, 128, ho, wo, generator=g), dtype), dtype, device, ld=128 + 16, c_off=8) if form == "B" else None
    assert form in C2f.fuse_front_forms and blk.front_fusable(prod, 0 if od is None else 128, dtype)  # both forms of Drone-YOLO-s are dispatched
    on = H.LaunchPlan()
    with H.record(on):
        got = blk(xd, front=(prod, od))
    off = H.LaunchPlan()
    with H.record(off):
        mid = prod(xd)
        layerwise = blk(mid if od is None else Concat()([mid, od]))
    torch.cuda.synchronize()
    assert entries(on).count(ENTRY) == 1 and ENTRY not in entries(off), (entries(on), entries(off))
    assert len(entries(on)) < len(entries(off))
    check_close(back(got), back(layerwise), dtype, f"form {form} {shape}: front fused vs two launches")
    # the fused launch sums as its two launches do (3x3: chunks, taps in order from the bias; 1x1: K ascending from zero, bias last)
    assert torch.equal(got.contiguous().view(torch.int16), layerwise.contiguous().view(torch.int16)), "fused front is not bit-identical to the two-launch path"


def test_whole_model_front_fusion_is_bit_identical_and_planned(device):
    """Drone-YOLO-s (nc 10), B = 2, 64 x 64, fp16: pred and the NMS rows with the front fusion on equal those with it off, bit for bit; the
    recorded plan holds two launches of the new entry and none of layers 3 and 19."""
    import drone_yolo_amd as D
    from drone_yolo_amd.engine.predictor import DetectionPredictor
    from drone_yolo_amd.utils.parity import seeded_state_dict

    model = D.DetectionModel(load_yaml("yolov8-p2-repvgg.yaml", "s", 10), nc=10, verbose=False)
    model.load_state_dict(seeded_state_dict(model.state_dict(), 8, cls_bias=-1.6))
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(8)).to(device)
    res = {}
    for on in (True, False):
        model.fuse_front = on
        pred = DetectionPredictor(model, dict(conf=0.25, iou=0.7, dtype=torch.float16, device=0))
        cf = pred.forward_device(x)
        torch.cuda.synchronize()
        res[on] = (cf.pred.clone(), cf.nms.out.clone(), cf.nms.count.clone(), entries(cf.plan), [t[0] for t in cf.plan.tags if t is not None])
    model.fuse_front = True
    (p1, o1, c1, e1, l1), (p0, o0, c0, e0, l0) = res[True], res[False]
    assert e1.count(ENTRY) == 2 and ENTRY not in e0, (e1.count(ENTRY), e0.count(ENTRY))
    assert 3 not in l1 and 19 not in l1 and 20 not in l1 and 3 in l0 and 19 in l0
    assert len(e1) == len(e0) - 2
    assert int(c1.sum()) > 0, "the fixture keeps no detection"
    assert torch.equal(p1, p0), f"pred differs: max|d| {float((p1 - p0).abs().max())}"
    assert torch.equal(c1, c0) and torch.equal(o1, o0), "NMS rows differ"


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("form", ["A", "B"])
def test_five_runs_beside_another_stream_are_bit_identical(form, dtype, device):
    case = front_case(form, 3, 33, 31, dtype)
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
        out, _, keep = run_front(case, dtype, device)
        assert H.last_kernel_name().startswith(KERNEL), H.last_kernel_name()
        torch.cuda.synchronize()
        outs.append(out.cpu().clone())
    check_close(back(outs[0]), case[4], dtype, f"c2f front form {form} 3x33x31 beside a second stream")
    for k in range(1, 5):
        assert torch.equal(outs[k].view(torch.int16), outs[0].view(torch.int16)), f"run {k} differs from run 0"
