"""GPU: ``dy_seg_loss`` over the cases of tests/_seg_loss_util.py against the float64 restatement (tests/test_seg_loss_host.py shows on the
CPU that the restatement reproduces the real reference, that the kernel's crop arithmetic equals the reference's crop masks, and that these
checks catch the ten mutants), plus the two small kernels of the Segment head's backward.

Per case: ``H.detection_loss(..., want_owner=True)`` on the case's head maps, whose owner map must EQUAL the real reference's
(tests/golden/seg_loss.npz) at every anchor, then ``H.seg_loss(..., want_grad=True)`` behind it: seg, its contribution to the total and
the gradients w.r.t. coefficient maps and prototypes within the case's bars (16 x the fp32 reference's own error against its float64 run).
``thin`` feeds its hand-made owner map (tests/_seg_loss_util.py says why).  Coefficient maps sit at the case's pitch (32, 36, 40) with NaN in
the padding lanes of the inputs; index maps are uint8 or int32, prototypes fp32 or bf16 as the case says.
"""
import pytest
import torch

from drone_yolo_amd import hip_ops as H
from tests import _seg_loss_util as U
from tests.test_seg_gpu import _report

pytestmark = pytest.mark.gpu


def _views(maps, device, ld=None, dtype=torch.float32):
    out = []
    for f in maps:
        n, c, h, w = f.shape
        buf = H.alloc_nhwc(n, ld or c, h, w, dtype, device)
        buf.fill_(float("nan"))
        lv = buf[:, :c]
        lv.copy_(f.to(device))
        out.append(lv)
    return out


def _inputs(case, device):
    if case["owner"] is not None:
        owner = case["owner"].to(device, torch.int32).contiguous()
    else:
        _, owner = H.detection_loss(_views(case["feats"], device), case["gt"].to(device), case["strides"], case["nc"], topk=case["topk"], want_owner=True)
    coefs = _views(case["coefs"], device, case["ld"])
    proto = _views([case["proto"]], device, dtype=case["proto_dtype"])[0]
    return owner, coefs, proto, case["masks"].to(device)


def _call(case, device, want_grad=True, buffers=None, inputs=None):
    owner, coefs, proto, masks = inputs or _inputs(case, device)
    r = H.seg_loss(owner, case["gt"].to(device), coefs, proto, masks, case["hw"], box=U.GAINS[0], topk=case["topk"], want_grad=want_grad, buffers=buffers)
    torch.cuda.synchronize()
    return owner, r


@pytest.mark.parametrize("cid", U.ALL_IDS)
def test_seg_loss(cid, device):
    case, ref_owner, _ = U.case_reference(cid)
    owner, (out, gcoef, gproto) = _call(case, device)
    assert torch.equal(owner.cpu().long(), ref_owner), f"{cid}: the device's owner map differs from the reference's at {(owner.cpu().long() != ref_owner).nonzero().tolist()[:8]}"
    gc, gp = [g.cpu().contiguous() for g in gcoef], gproto.cpu().contiguous()
    for g, c in zip(gcoef, case["coefs"]):
        assert tuple(g.shape) == tuple(c.shape) and g.stride(3) == case["ld"]
    assert tuple(gp.shape) == tuple(case["proto"].shape)
    res = U.check_result(cid, out.cpu(), gc, gp)
    _report(f"seg_loss {cid}", {k: v for k, v in res.items() if k != "ok"})
    assert bool(torch.isfinite(out).all()) and all(bool(torch.isfinite(g).all()) for g in (*gc, gp))
    assert res["items_err"] <= res["items_bar"], f"{cid}: seg {out.tolist()} is {res['items_err']:.2e} from float64, bar {res['items_bar']:.2e}"
    assert res["grad_err"] <= res["grad_bar"], f"{cid}: gradients are {res['grad_err']:.2e} of the largest entry from float64, bar {res['grad_bar']:.2e}"
    bg = (owner.cpu() < 0)
    pm = torch.cat([g.reshape(g.shape[0], U.NM, -1) for g in gc], 2)
    assert not bool(pm.permute(0, 2, 1)[bg].any())  # background rows are exactly zero
    # the value-only call gives the same two numbers and writes no gradient
    _, out2 = _call(case, device, want_grad=False)
    assert torch.equal(out2.cpu(), out.cpu())


@pytest.mark.parametrize("cid", ["conv-C4", "crowd", "ld36-C3"])
def test_second_call_on_the_same_buffers_is_bit_equal(cid, device):
    case = U.case_reference(cid)[0]
    inputs, bufs = _inputs(case, device), {}
    _, (out, gcoef, gproto) = _call(case, device, buffers=bufs, inputs=inputs)
    first = [out.clone(), *[g.clone() for g in gcoef], gproto.clone()]
    _, (out, gcoef, gproto) = _call(case, device, buffers=bufs, inputs=inputs)
    for a, b in zip(first, [out, *gcoef, gproto]):
        assert torch.equal(a, b)  # no atomics: the same bits (NaN nowhere: equal would fail)
    # and a call with fresh buffers too
    _, (out3, gcoef3, gproto3) = _call(case, device, inputs=inputs)
    for a, b in zip(first, [out3, *gcoef3, gproto3]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("cid", ["none", "half"])
def test_every_gradient_element_is_written(cid, device):
    case, _, (seg, contrib, rc, rp) = U.case_reference(cid)
    inputs, bufs = _inputs(case, device), {}
    _call(case, device, buffers=bufs, inputs=inputs)
    for g in (*bufs["gcoef"], bufs["gproto"]):
        g.fill_(float("nan"))
    bufs["out"].fill_(float("nan"))
    _, (out, gcoef, gproto) = _call(case, device, buffers=bufs, inputs=inputs)
    assert all(bool(torch.isfinite(g).all()) for g in (out, *gcoef, gproto))
    res = U.check_result(cid, out.cpu(), [g.cpu() for g in gcoef], gproto.cpu())
    assert res["ok"], res
    if cid == "none":
        assert float(out[0]) == 0 and float(out[1]) == 0 and not any(bool(g.any()) for g in (*gcoef, gproto))
    else:
        assert not bool(gproto[1].any()) and bool(gproto[0].any())  # the image without labels gets zeros, the other one its gradient


def test_host_refusals(device):
    case = U.case_reference("conv-C3")[0]
    owner, coefs, proto, masks = _inputs(case, device)
    gt = case["gt"].to(device)
    with pytest.raises(ValueError, match="prototype grid"):  # ratio 3
        H.seg_loss(owner, gt, coefs, H.alloc_nhwc(2, 32, 48, 48, torch.float32, device), masks, case["hw"])
    with pytest.raises(NotImplementedError, match="nm"):
        H.seg_loss(owner, gt, [c[:, :16] for c in coefs], proto[:, :16], masks, case["hw"])
    with pytest.raises(TypeError, match="overlap"):  # one float mask per label
        H.seg_loss(owner, gt, coefs, proto, torch.zeros(8, 16, 16, device=device), case["hw"])
    with pytest.raises(ValueError, match="owner"):
        H.seg_loss(owner[:, :-1].contiguous(), gt, coefs, proto, masks, case["hw"])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_space_to_depth_inverts_depth_to_space(dtype, device):
    g = torch.Generator().manual_seed(3)
    x = H.alloc_nhwc(2, 32, 5, 7, dtype, device)  # (n, 4c, h, w) with c = 8: odd sizes, more than one block
    x.copy_(torch.randn(2, 32, 5, 7, generator=g).to(device))
    up = H.depth_to_space2(x)
    back = H.space_to_depth2(up)
    torch.cuda.synchronize()
    assert tuple(up.shape) == (2, 8, 10, 14) and tuple(back.shape) == tuple(x.shape)
    assert torch.equal(back, x)  # a pure move: the round trip is the input, bit for bit
    ref = x.cpu().float().reshape(2, 2, 2, 8, 5, 7).permute(0, 3, 4, 1, 5, 2).reshape(2, 8, 10, 14)
    assert torch.equal(up.cpu().float(), ref)
    big = H.alloc_nhwc(3, 16, 34, 46, dtype, device)
    big.copy_(torch.randn(3, 16, 34, 46, generator=g).to(device))
    assert torch.equal(H.depth_to_space2(H.space_to_depth2(big)), big)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_grad_cast_scaled(dtype, device):
    g = torch.Generator().manual_seed(4)
    src = torch.randn(3, 32, 9, 11, generator=g)
    view = _views([src], device, ld=40)[0]
    scale = torch.tensor([0.37], device=device)
    for s in (None, scale):
        dz = H.grad_cast_scaled(view, dtype, scale=s)
        torch.cuda.synchronize()
        want = (src * torch.tensor(0.37 if s is not None else 1.0, dtype=torch.float32)).to(dtype)
        assert dz.dtype == dtype and tuple(dz.shape) == tuple(src.shape) and dz.stride(1) == 1
        assert torch.equal(dz.cpu(), want), float((dz.cpu().float() - want.float()).abs().max())  # one fp32 multiply, one rounding: exact
    with pytest.raises(RuntimeError):
        H.grad_cast_scaled(H.alloc_nhwc(1, 12, 2, 2, torch.float32, device), dtype)  # c % 8 != 0
