"""GPU: ``dy_detection_loss`` over the label-geometry and converged-head sweep of tests/_loss_util.py against the float64 reference
(tests/test_loss_geometry_host.py shows on the CPU that every case is sound and that these checks catch a non-strict in-box test, the
last index on overlap ties, an arg-max over claimants only, topk - 1 picks, per-box maxima over picks, a missing DFL clamp, h / w swapped
in the anchor index, an attached alpha and a box loss in pixels).

Per case, one ``H.detection_loss(..., want_owner=True, want_grad=True)`` call (value only for k1 / k13):
* assignment: the owner map equals ``assign64``'s outside the unsure set (DELTA = 1.76e-3, empty in every case for the reference itself),
  inside it one of the candidates; background rows are exactly -1;
* value and gradient: against ``loss_from_owner64`` and float64 autograd through it UNDER THE DEVICE'S owner map; every element finite;
* bars: 16 x the fp32 oracle's own error against float64 on that case (items: relative, floor 0.05 on the reference; gradient: relative
  to the level's largest entry), never below 16 fp32 ulps and never above the 2e-4 / 1e-4 of tests/test_loss_gpu.py.

Measured on an MI355X (fg = foreground anchors of the device's owner map; unsure = size of the unsure set, 0 everywhere: the device's
owner map equals assign64's at every anchor of every case; "oracle" = fp32 oracle against float64 on the host, "device" = the kernel
against float64, "bar" = what is asserted):

    case      fg   items: oracle  device  bar       gradient: oracle  device  bar
    edge-R    65   1.5e-07 5.3e-08 2.4e-06          3.7e-07 4.4e-07 5.9e-06
    edge-C   120   5.2e-07 7.6e-07 8.4e-06          2.9e-06 2.5e-06 4.6e-05   (the same at pitches 74, 76, 80, 88)
    sliver-R  15   8.3e-08 3.9e-08 1.9e-06          8.8e-08 8.8e-08 1.9e-06
    sliver-C  25   8.4e-07 5.2e-07 1.4e-05          4.2e-06 3.8e-06 6.7e-05
    whole-R   35   5.4e-07 9.4e-08 8.7e-06          1.5e-06 9.8e-07 2.4e-05
    whole-C   40   1.0e-06 4.7e-07 1.6e-05          2.2e-06 2.7e-06 3.5e-05
    dup-R     55   3.1e-07 2.8e-07 5.0e-06          9.4e-07 1.1e-06 1.5e-05
    dup-C     79   7.8e-07 9.4e-07 1.2e-05          2.0e-06 2.4e-06 3.3e-05
    crowd-C   83   2.9e-07 3.8e-07 4.6e-06          2.3e-06 2.4e-06 3.7e-05
    pad-R    111   1.7e-07 1.7e-07 2.7e-06          4.4e-07 5.4e-07 7.1e-06
    gmax0-R    0   3.2e-08 3.2e-08 1.9e-06          8.4e-08 8.4e-08 1.9e-06
    clamp-C   40   3.5e-07 2.0e-07 5.6e-06          3.6e-06 2.0e-06 5.8e-05
    rect-R    68   4.4e-07 3.5e-07 7.1e-06          4.5e-07 7.6e-07 7.3e-06
    rect-C    70   6.2e-07 7.6e-07 9.9e-06          2.7e-06 2.2e-06 4.4e-05
    nc1-R     66   2.8e-07 2.8e-07 4.4e-06          3.0e-07 3.5e-07 4.8e-06
    nc3-R     69   2.6e-07 3.1e-07 4.2e-06          5.3e-07 9.4e-07 8.5e-06   (the same at pitches 67, 68, 72, 76, 80, 88)
    nc80-R    70   1.6e-07 3.2e-07 2.6e-06          3.0e-07 6.8e-07 4.8e-06
    lv3-C     57   7.9e-07 4.3e-07 1.3e-05          2.4e-06 1.2e-06 3.9e-05
    k1-R      10   8.3e-08 6.6e-08 1.9e-06          value only
    k13-R    110   7.8e-08 6.6e-07 1.9e-06          value only
    peak      40   1.0e-06 8.1e-07 1.6e-05          3.3e-06 2.1e-06 5.3e-05
    ties      29   1.4e-07 1.4e-07 2.2e-06          1.7e-07 1.7e-07 2.6e-06
    tiny       2   2.6e-06 4.5e-06 4.1e-05          2.3e-05 1.9e-05 1.0e-04

No case needs more than 16 x: the device sits at 0.2 .. 8 times the oracle's own error (k13-R, whose oracle error is below one fp32 ulp
and whose bar is the floor of 16 ulps, is the 8), two orders of magnitude below the 2e-4 / 1e-4 of tests/test_loss_gpu.py.  The oracle
columns are measured on the host at run time and move a little from host to host.
"""
import pytest
import torch

from drone_yolo_amd import hip_ops as H
from tests import _loss_util as U
from tests.test_seg_gpu import _report

pytestmark = pytest.mark.gpu


def _levels(feats, device, ld=None):
    """NHWC views at pixel pitch ``ld``; the padding lanes hold NaN (nothing may read them)."""
    out = []
    for f in feats:
        n, c, h, w = f.shape
        buf = H.alloc_nhwc(n, ld or c, h, w, torch.float32, device)
        buf.fill_(float("nan"))
        lv = buf[:, :c]
        lv.copy_(f.to(device))
        assert H.view_params(lv)[1] == (ld or c)
        out.append(lv)
    return out


def _run(cid, device, ld=None):
    case, asg, _, _ = U.case_reference(cid)
    r = H.detection_loss(_levels(case["feats"], device, ld), case["gt"], case["strides"], case["nc"], topk=case["topk"], want_owner=True, want_grad=case["grad"])
    torch.cuda.synchronize()
    out, owner = r[0].cpu(), r[1].cpu().long()
    grads = None
    if case["grad"]:
        for g, f in zip(r[2], case["feats"]):
            assert tuple(g.shape) == tuple(f.shape) and H.view_params(g)[1] == (ld or f.shape[1])  # the values only: nothing reads a gradient's padding
        grads = [g.cpu().contiguous() for g in r[2]]
    res = U.check_case(cid, owner, out, grads)
    _report(f"detection_loss geometry {cid}" + (f" ld={ld}" if ld else ""), {k: v for k, v in res.items() if not k.startswith("ok")})
    G = case["gt"].shape[1]
    assert bool(((owner >= -1) & (owner < max(G, 1))).all()) and (G > 0 or bool((owner == -1).all()))
    assert bool(torch.isfinite(out).all()), out
    assert res["ok_owner"], f"{cid}: {res['owner_wrong']} owners differ from assign64 outside the unsure set, {res['unsure_wrong']} inside it are no candidate"
    assert res["ok_items"], f"{cid}: items {out.tolist()} are {res['items_err']:.2e} from float64, bar {res['items_bar']:.2e} (oracle {res['oracle_items']:.2e})"
    assert res["ok_grad"], f"{cid}: gradient is {res['grad_err']:.2e} of the largest entry from float64, bar {res['grad_bar']:.2e} (oracle {res['oracle_grad']:.2e})"
    return case, owner, out, grads


@pytest.mark.parametrize("cid", U.CASE_IDS)
def test_detection_loss_geometry(cid, device):
    case, owner, out, grads = _run(cid, device)
    if cid == "gmax0-R":  # no labels at all: every row is background, the gradient is sigmoid(x) * cls_gain * B
        assert float(out[0]) == 0.0 and float(out[2]) == 0.0
        for g, f in zip(grads, case["feats"]):
            assert bool((g[:, : 4 * U.REG] == 0).all())
            exp = f[:, 4 * U.REG :].double().sigmoid() * U.GAINS[1] * f.shape[0]
            assert float((g[:, 4 * U.REG :].double() - exp).abs().max()) <= 16 * U.F32_EPS * float(exp.max())
    if cid == "peak":  # +-50 logits on background anchors: sigmoid(50) = 1, sigmoid(-50) = 1.9e-22, neither 0 nor NaN nor a denormal flush
        tss = U.loss_from_owner64(case["feats"], case["gt"], owner, case["strides"], case["nc"], want_grad=False)[3]["tss"]
        k, a0, n = U.GAINS[1] * case["gt"].shape[0] / tss, 0, 0
        for g, f in zip(grads, case["feats"]):
            hw = f.shape[2] * f.shape[3]
            bg = (owner[:, a0 : a0 + hw] < 0).reshape(f.shape[0], 1, f.shape[2], f.shape[3])
            x = f[:, 4 * U.REG :]
            sel = (x.abs() == 50) & bg
            exp = x.double().sigmoid() * k
            assert bool(((g[:, 4 * U.REG :].double() - exp).abs()[sel] <= 16 * U.F32_EPS * exp[sel]).all())
            a0, n = a0 + hw, n + int(sel.sum())
        assert n > 0


@pytest.mark.parametrize("cid,ld", U.PITCH_CASES)
def test_detection_loss_pixel_pitches(cid, ld, device):
    """Head maps and gradient maps at other pixel pitches: the 16-byte-aligned decode path (pitch a multiple of 4) and the whole-row
    gradient path (pitch a multiple of 4 with fewer than 8 floats of padding: 76 and 80 at nc = 10, 68 at nc = 3)."""
    _run(cid, device, ld)
