"""GPU: ``dy_obb_loss`` over the cases of tests/_obb_loss_util.py against the float64 restatement (tests/test_obb_loss_host.py shows on the
CPU that every case is sound, that the restatement reproduces the real reference, and that these checks catch the nine mutants).

Per case, one ``H.obb_loss(..., want_owner=True, want_grad=True)`` call (value only for clampov and big):
* assignment: the owner map equals ``assign64_rot``'s outside the unsure set, inside it one of the candidates; background rows are exactly -1.
  The unsure set is empty in every case (membership is pinned by the fp32 restatement of the in-box arithmetic, tests/_obb_loss_util.py), so
  this is equality at every anchor -- and, by the host test, equality with the REAL reference's fp32 owner map, asserted here as well:
  ``edge``'s r = pi/2 labels, whose edges and corners carry anchor centres, are decided as the reference decides them;
* value and gradients (head maps and angle-logit maps) against ``loss_from_owner64_rot`` and float64 autograd through it UNDER THE DEVICE'S
  owner map; every element finite; the angle gradient of a background anchor is exactly 0;
* bars: 16 x the real reference's fp32 error against float64 on that case, never below 16 fp32 ulps, never above 2e-4 / 1e-4.

Head maps sit at pitch 80 (nc 10: the whole-row gradient path) and angle maps at pitch 8 (the prediction head's ANGLE_COUT) with NaN in the
padding of the inputs; ``conv`` and ``nc80`` use the unpadded pitches.
"""
import pytest
import torch

from drone_yolo_amd import hip_ops as H
from tests import _obb_loss_util as U
from tests.test_seg_gpu import _report

pytestmark = pytest.mark.gpu


def _views(maps, device, ld):
    """NHWC views at pixel pitch ``ld`` (None: the channel count); the padding lanes hold NaN (nothing may read them)."""
    out = []
    for f in maps:
        n, c, h, w = f.shape
        buf = H.alloc_nhwc(n, ld or c, h, w, torch.float32, device)
        buf.fill_(float("nan"))
        lv = buf[:, :c]
        lv.copy_(f.to(device))
        out.append(lv)
    return out


def _pitches(case):
    return (None, None) if case["id"] in ("conv", "nc80") else (-(-(64 + case["nc"]) // 16) * 16, 8)


def _call(case, device, want_grad, buffers=None):
    ld, lda = _pitches(case)
    gt = case["gt"].to(device) if case["device_table"] else case["gt"]
    r = H.obb_loss(_views(case["feats"], device, ld), _views(case["angles"], device, lda), gt, case["strides"], case["nc"], topk=case["topk"], want_owner=True,
                   want_grad=want_grad, buffers=buffers)
    torch.cuda.synchronize()
    return r


def _run(cid, device):
    case, asg, _, _ = U.case_reference(cid)
    r = _call(case, device, case["grad"])
    out, owner = r[0].cpu(), r[1].cpu().long()
    grads = agrads = None
    if case["grad"]:
        grads, agrads = [g.cpu().contiguous() for g in r[2]], [g.cpu().contiguous() for g in r[3]]
        for g, f, ga, an in zip(grads, case["feats"], agrads, case["angles"]):
            assert tuple(g.shape) == tuple(f.shape) and tuple(ga.shape) == tuple(an.shape)
    res = U.check_case(cid, owner, out, grads, agrads)
    _report(f"obb_loss {cid}", {k: v for k, v in res.items() if not k.startswith("ok")})
    G = case["gt"].shape[1]
    assert bool(((owner >= -1) & (owner < max(G, 1))).all()) and (G > 0 or bool((owner == -1).all()))
    assert bool(torch.isfinite(out).all()), out
    assert res["unsure"] == 0 and torch.equal(owner, U.golden(cid)["owner"]), f"{cid}: owners differ from the real reference's at {(owner != U.golden(cid)['owner']).nonzero().tolist()}"
    assert res["ok_owner"], f"{cid}: {res['owner_wrong']} owners differ from assign64_rot outside the unsure set, {res['unsure_wrong']} inside it are no candidate"
    assert res["ok_items"], f"{cid}: items {out.tolist()} are {res['items_err']:.2e} from float64, bar {res['items_bar']:.2e} (reference {res['oracle_items']:.2e})"
    assert res["ok_grad"], (f"{cid}: gradient is {res['grad_err']:.2e} of the largest entry from float64 (head {res['head_grad_err']:.2e}, angle {res['angle_grad_err']:.2e}), "
                            f"bar {res['grad_bar']:.2e} (reference {res['oracle_grad']:.2e})")
    return case, owner, out, grads, agrads


@pytest.mark.parametrize("cid", U.CASE_IDS)
def test_obb_loss(cid, device):
    case, owner, out, grads, agrads = _run(cid, device)
    if grads is None:
        return
    a0 = 0
    for g, ga, f in zip(grads, agrads, case["feats"]):  # background anchors: zero box bins, zero angle gradient, exactly
        hw = f.shape[2] * f.shape[3]
        bg = (owner[:, a0 : a0 + hw] < 0).reshape(f.shape[0], f.shape[2], f.shape[3])
        assert bool((ga[:, 0][bg] == 0).all()) and bool((g[:, : 4 * U.REG].permute(0, 2, 3, 1)[bg] == 0).all())
        a0 += hw
    if cid == "none":  # no label in the batch: box and DFL terms 0, angle gradient exactly zero, class gradient dense
        assert float(out[0]) == 0.0 and float(out[2]) == 0.0
        for g, ga, f in zip(grads, agrads, case["feats"]):
            assert not bool(ga.any())
            exp = f[:, 4 * U.REG :].double().sigmoid() * U.GAINS[1] * f.shape[0]
            assert float((g[:, 4 * U.REG :].double() - exp).abs().max()) <= 16 * U.F32_EPS * float(exp.max())


@pytest.mark.parametrize("cid", ["rand", "none", "pad"])
def test_value_only_call_and_second_call_on_the_same_buffers(cid, device):
    """``want_grad=False`` gives the same scalars; a second call on the SAME output, workspace and gradient buffers -- filled with NaN in
    between for the gradient maps, left as the first call left it for the workspace -- gives bit-identical outputs: nothing depends on stale
    workspace, and both gradient maps are rewritten completely (the angle map's padding channels included)."""
    case = U.build_case(cid)
    bufs = {}
    first = _call(case, device, True, bufs)
    keep = [first[0].clone(), first[1].clone(), [g.clone() for g in first[2]], [g.clone() for g in first[3]]]
    raw = [torch.as_strided(g, (g.shape[0], g.shape[2], g.shape[3], H.view_params(g)[1]), (g.stride(0), g.stride(2), g.stride(3), 1)) for g in first[3]]
    raw_keep = [t.clone() for t in raw]
    for g in (*bufs["grads"], *raw):
        g.fill_(float("nan"))
    bufs["out"].fill_(float("nan"))
    second = _call(case, device, True, bufs)
    assert second[0].data_ptr() == first[0].data_ptr() and second[3][0].data_ptr() == first[3][0].data_ptr()
    assert torch.equal(second[0], keep[0]) and torch.equal(second[1], keep[1])
    for a, b in zip((*second[2], *raw), (*keep[2], *raw_keep)):
        assert torch.equal(a, b)  # NaN != NaN: a hole would show
    for t in raw:
        assert not bool(t[..., 1:].any())  # whole rows: zeros behind the value
    value = _call(case, device, False)
    assert len(value) == 2 and torch.equal(value[0], keep[0]) and torch.equal(value[1], keep[1])


def test_refusals(device):
    case = U.build_case("rand")
    feats, angles = _views(case["feats"], device, None), _views(case["angles"], device, None)
    with pytest.raises(ValueError, match=r"\(N, gmax, 6\)"):
        H.obb_loss(feats, angles, case["gt"][..., :5], case["strides"], case["nc"])
    with pytest.raises(ValueError, match="one angle map per level"):
        H.obb_loss(feats, angles[:2], case["gt"], case["strides"], case["nc"])
    with pytest.raises(RuntimeError, match="reg_max"):
        H.obb_loss(feats, angles, case["gt"], case["strides"], case["nc"] + 4 * 16 - 4 * 8, reg_max=8)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_angle_grad_cast_scales_and_pads(dtype, device):
    """``dy_obb_angle_grad_cast`` (the angle tail's dz under the trainer's lazy seed): channel 0 of a pitch-8 fp32 map times a DEVICE scalar
    other than 1 (fp16 training's seed is the loss scale), rounded once to the storage type; zeros in channels 1..7; no scale = times 1.  Odd
    map sizes, more rows than one block; the input's padding channels hold NaN (only channel 0 is read)."""
    g = torch.Generator().manual_seed(3)
    for n, h, w in ((2, 5, 7), (3, 16, 24)):
        buf = H.alloc_nhwc(n, 8, h, w, torch.float32, device)
        buf.fill_(float("nan"))
        val = torch.randn(n, 1, h, w, generator=g)
        buf[:, :1].copy_(val.to(device))
        for scale in (torch.tensor(3.0, device=device), torch.tensor(65536.0, device=device) if dtype != torch.float16 else torch.tensor(0.125, device=device), None):
            dz = H.obb_angle_grad_cast(buf[:, :1], dtype, scale=scale)
            torch.cuda.synchronize()
            assert dz.dtype == dtype and tuple(dz.shape) == (n, 8, h, w) and H.view_params(dz)[1] == 8
            exp = (val * (float(scale) if scale is not None else 1.0)).to(dtype)  # one rounding of the fp32 product
            assert torch.equal(dz[:, :1].cpu(), exp) and not bool(dz[:, 1:].any())
        plain = H.obb_angle_grad_cast(val.to(device), dtype, scale=torch.tensor(3.0, device=device))  # a contiguous (n, 1, h, w) gradient: pitch 1
        assert torch.equal(plain[:, :1].cpu(), (val * 3.0).to(dtype))
