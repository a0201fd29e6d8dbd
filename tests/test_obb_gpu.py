"""GPU parity of the oriented-box path against tests/golden/obb.npz (tools/make_obb_golden.py: the REAL reference's OBB head, dist2rbox,
``non_max_suppression(rotated=True)``, ``OBBPredictor.construct_result`` and end-to-end predictions).

Bars.  ``dy_obb_decode`` and every angle: within 8 x the reference's own fp32-vs-float64 difference on the decode fixture (``dec_tol`` in the
file: 2.7e-5 px on the centres, 2.3e-6 rad).  ``dy_nms_rotated``: the reference's kept anchors in order and its counts
EXACTLY -- the fixtures are ones the reference decides with a margin (no pair within M of iou_thres, M = 8 x max |iou32 - iou64|) -- rows
equal in fp32 (x, y, w, h, conf, cls are copies).  ``dy_scale_rboxes``: equal in fp32 (divisions and fmod are exact operations); the angle
within the tolerance above.  End to end: kept anchors, classes and order exact, IoU >= 0.999 of the unrotated boxes (the project's
detection bar), theta within the fixture's own ``theta_tol`` (8 x the difference of the reference's fp32 and float64 runs on these inputs).
"""
import functools
import math

import numpy as np
import pytest
import torch

from drone_yolo_amd import YOLO, _lib
from drone_yolo_amd import hip_ops as H
from drone_yolo_amd.nn import modules as M
from drone_yolo_amd.nn.tasks import OBBModel, initialize_weights
from drone_yolo_amd.utils import ops
from oracle import drone_yolo_oracle as O
from tests import _obb_util as U
from tests._util import box_iou_pairs, golden, load_yaml, meta, split_rows
from tests.test_model_gpu import RTOL as _RTOL
from tests.test_model_gpu import _report as _parity_report

pytestmark = pytest.mark.gpu
X2 = H.F16X2
RTOL = {**_RTOL, X2: _RTOL[torch.float32]}  # split float16 (22 mantissa bits) is held to fp32's


@pytest.fixture(scope="module")
def g():
    return golden("obb.npz")


def _report(name, payload):
    _parity_report(name, payload)
    print(name, payload)


def _randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ---- head ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, X2, torch.float16, torch.bfloat16], ids=["f32", "split", "f16", "bf16"])
def test_head_matches_reference_vectors(g, dtype, device):
    M.OBB.legacy = True
    head = M.OBB(nc=10, ne=1, ch=(32, 64))
    head.load_state_dict(O.seeded_state_dict(head.state_dict(), int(g["head_seed"])))
    initialize_weights(head)
    head = head.to(device).eval()
    head.stride = torch.tensor([8.0, 16.0])
    s = int(g["head_xseed"])
    xs = [H.to_nhwc(_randn(s, 2, 32, 8, 12).to(device), dtype), H.to_nhwc(_randn(s + 1, 2, 64, 4, 6).to(device), dtype)]
    y, (feats, angle) = head(xs)
    assert tuple(y.shape) == (2, 4 + 10 + 1, 120) and tuple(angle.shape) == (2, 1, 120) and len(feats) == 2 and torch.equal(y[:, 14:], angle)
    for name, got, ref in (("OBB y", y[:, :14], g["head_y"]), ("OBB angle", angle, g["head_angle"])):
        ref = torch.from_numpy(ref)
        err, scale = float((got.float().cpu() - ref).abs().max()), float(ref.abs().max())
        _report(name, {"dtype": str(dtype), "max_abs_err": err, "scale": scale})
        assert err <= RTOL[dtype] * scale, f"{name} [{dtype}]: max|err| {err:.4e}, scale {scale:.3f}"
    head.fuse_tail = True  # the predictor's form: nothing concatenated
    try:
        y2, (none, theta, levels) = head(xs)
    finally:
        head.fuse_tail = False
    assert none is None and tuple(y2.shape) == (2, 14, 120) and tuple(theta.shape) == (2, 120) and torch.equal(theta, angle[:, 0]) and torch.equal(y2, y[:, :14])
    assert [tuple(l.shape) for l in levels] == [(2, 1, 8, 12), (2, 1, 4, 6)] and all(l.dtype == torch.float32 for l in levels)
    head.train()
    with pytest.raises(NotImplementedError):
        head(xs)


# ---- dy_obb_decode ----------------------------------------------------------------------------------------------------------------
def test_obb_decode_against_float64(g, device):
    dist, logits, anchors, strides = U.decode_inputs(int(g["dec_seed"]))
    B, nc = U.DECODE_BATCH, U.DECODE_NC
    A = anchors.shape[0]
    xywh = U.detect_xywh(dist, anchors, strides)
    scores = torch.rand(B, nc, A, generator=torch.Generator().manual_seed(5))
    pred0 = torch.cat((xywh, scores), 1).contiguous()
    pred = pred0.to(device)
    levels = []
    for (h, w, s, ld), lg in zip(U.DECODE_LEVELS, logits):  # the angle maps: channel 0 of a buffer with pixel pitch ld, the rest poison
        buf = torch.full((B, h, w, ld), 1e30, dtype=torch.float32, device=device)
        buf[..., 0] = lg.to(device)
        levels.append(buf.permute(0, 3, 1, 2)[:, :1])
    guard = 16  # 64 bytes either side of theta
    tbuf = torch.full((B * A + 2 * guard,), -7.0, dtype=torch.float32, device=device)
    theta = tbuf[guard : guard + B * A].view(B, A)
    out = H.obb_decode(levels, [l[2] for l in U.DECODE_LEVELS], pred, nc, theta=theta)
    assert out.data_ptr() == theta.data_ptr()
    tol_xy, tol_th = (float(v) for v in g["dec_tol"])
    got, th = pred.cpu(), theta.cpu()
    e_xy = float((got[:, :2].double() - torch.from_numpy(g["dec_xy64"])).abs().max())
    e_th = float((th.double() - torch.from_numpy(g["dec_theta64"])).abs().max())
    _report("dy_obb_decode", {"max_err_xy": e_xy, "tol_xy": tol_xy, "max_err_theta": e_th, "tol_theta": tol_th})
    assert e_xy <= tol_xy and e_th <= tol_th
    assert torch.equal(got[:, 2:], pred0[:, 2:]), "rows 2.. of pred must be untouched"
    assert bool((tbuf[:guard] == -7.0).all()) and bool((tbuf[guard + B * A :] == -7.0).all()), "theta's guard bytes were written"
    first = np.cumsum([0] + [h * w for h, w, _, _ in U.DECODE_LEVELS])  # first / last anchor of every level: the saturated logits
    lo, hi = -0.25 * math.pi, 0.75 * math.pi
    for a0, a1 in zip(first[:-1], first[1:] - 1):
        if a0 != a1:  # (the 1 x 1 level holds one anchor: its second assignment wins)
            assert abs(float(th[0, a0]) - lo) <= tol_th and abs(float(th[1, a0]) - hi) <= tol_th
        assert abs(float(th[0, a1]) - hi) <= tol_th and abs(float(th[1, a1]) - lo) <= tol_th and abs(float(th[2, a1]) - 0.25 * math.pi) <= tol_th


# ---- dy_nms_rotated ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _nms_case(name):
    g = golden("obb.npz")
    pred, theta = U.nms_inputs(name, int(g[f"nms_{name}__seed"]))
    return pred, theta, dict(U.NMS_CASES[name][3])


def _run_nms(pred, theta, kw, device, bufs=None, prefiltered=False):
    kw = dict(kw)
    mask = None
    if kw.get("classes") is not None:
        mask = torch.zeros(U.NC, dtype=torch.uint8)
        mask[kw.pop("classes")] = 1
        mask = mask.to(device)
    kw.pop("classes", None)
    return H.nms_rotated(pred, theta, U.CONF, U.IOU, nc=U.NC, classes_mask=mask, bufs=bufs, prefiltered=prefiltered,
                         **{"max_det": 300, **kw})


@pytest.mark.parametrize("name", list(U.NMS_CASES))
def test_nms_rotated_against_the_reference(g, name, device):
    assert int(_lib.lib().dy_nms_rotated_lds_cap()) == U.LDS_CAP
    pred, theta, kw = _nms_case(name)
    pd, td = pred.to(device), theta.to(device)
    bufs = _run_nms(pd, td, kw, device)
    counts = [int(k) for k in g[f"nms_{name}__n"]]
    max_det = kw.get("max_det", 300)
    assert tuple(bufs.out.shape) == (len(counts), max_det, 7)
    assert bufs.count.tolist() == counts, f"{name}: kept {bufs.count.tolist()}, the reference {counts}"
    exp_idx, exp_rows = split_rows(g[f"nms_{name}__idx"], counts), split_rows(g[f"nms_{name}__rows"], counts)
    out, index = bufs.out.cpu().numpy(), bufs.index.cpu().numpy()
    tol_th = float(g["dec_tol"][1])
    for b, k in enumerate(counts):
        assert np.array_equal(index[b, :k], exp_idx[b]), f"{name}: image {b} keeps other anchors than the reference"
        assert (index[b, k:] == -1).all() and (out[b, k:] == 0).all(), "rows behind the count must be zero, their index -1"
        # the reference's row is (x, y, w, h, conf, cls, theta); ours (x, y, w, h, theta, conf, cls)
        assert np.array_equal(out[b, :k, :4], exp_rows[b][:, :4]) and np.array_equal(out[b, :k, 5:7], exp_rows[b][:, 4:6])
        assert np.abs(out[b, :k, 4] - exp_rows[b][:, 6]).max(initial=0.0) <= tol_th
    # a second run into other buffers is byte-identical
    again = _run_nms(pd, td, kw, device)
    assert torch.equal(again.out.view(torch.int32), bufs.out.view(torch.int32)) and torch.equal(again.index, bufs.index) and torch.equal(again.count, bufs.count)


def test_nms_rotated_helper_and_non_max_suppression_route_to_the_kernel(g, device):
    pred, theta, kw = _nms_case("chunks")
    counts = [int(k) for k in g["nms_chunks__n"]]
    rows = ops.non_max_suppression(torch.cat((pred, theta[:, None]), 1).to(device), U.CONF, U.IOU, nc=U.NC, rotated=True)
    exp = split_rows(g["nms_chunks__rows"], counts)
    for r, e in zip(rows, exp):  # the reference's column order: x, y, w, h, conf, cls, angle
        assert tuple(r.shape) == e.shape and np.array_equal(r[:, :6].cpu().numpy(), e[:, :6])
    idx, boxes, scores = U.sorted_candidates(pred, theta, 3, {})
    keep = ops.nms_rotated(boxes.to(device), scores.to(device), U.IOU)
    assert np.array_equal(idx[keep.cpu()].numpy(), split_rows(g["nms_chunks__idx"], counts)[3])
    with pytest.raises(NotImplementedError):
        ops.non_max_suppression(torch.cat((pred, theta[:, None]), 1).to(device), U.CONF, U.IOU, nc=U.NC, rotated=True, multi_label=True)
    with pytest.raises(NotImplementedError, match="nc"):  # (without nc the reference takes the angle row for a class as well)
        ops.non_max_suppression(torch.cat((pred, theta[:, None]), 1).to(device), U.CONF, U.IOU, rotated=True)
    d = _lib.NmsDesc()  # the kernel itself refuses multi_label before any launch
    b = H.RNmsBuffers(1, 64, 300, device)
    d.pred, d.batch, d.nc, d.anchors, d.conf_thres, d.iou_thres, d.max_det, d.max_nms = pred.to(device).data_ptr(), 1, U.NC, 64, 0.25, 0.45, 300, 30000
    d.out, d.out_count, d.workspace, d.workspace_bytes, d.multi_label = b.out.data_ptr(), b.count.data_ptr(), b.workspace.data_ptr(), b.workspace.numel(), 1
    import ctypes
    assert _lib.lib().dy_nms_rotated(ctypes.byref(d), theta.to(device).data_ptr(), None) == -2  # DY_ERR_UNSUPPORTED


def test_nms_rotated_prefiltered_by_the_fused_detect_filter(device):
    """The candidate list the Detect decode's fused filter leaves in the workspace gives the same result as the kernel's own filter."""
    nc, reg_max, n = 3, 16, 2
    hw, strides = [(6, 10), (3, 5)], [8.0, 16.0]
    A = sum(h * w for h, w in hw)
    gen = torch.Generator().manual_seed(11)
    levels = []
    for h, w in hw:
        buf = H.alloc_nhwc(n, 4 * reg_max + nc, h, w, torch.float32, device, ld=68)
        buf.copy_(torch.randn(n, 4 * reg_max + nc, h, w, generator=gen).to(device))
        levels.append(buf)
    theta = ((torch.rand(n, A, generator=gen) - 0.25) * math.pi).to(device)
    fused = H.RNmsBuffers(n, A, 300, device)
    y = H.detect_decode(levels, strides, nc, reg_max, nms_bufs=fused, conf_thres=U.CONF)
    H.nms_rotated(y, theta, U.CONF, U.IOU, nc=nc, bufs=fused, prefiltered=True)
    plain = H.nms_rotated(y, theta, U.CONF, U.IOU, nc=nc)
    assert int(plain.count.sum()) >= 4, "the case must keep something"
    assert torch.equal(fused.count, plain.count) and torch.equal(fused.index, plain.index) and torch.equal(fused.out, plain.out)


def test_nms_rotated_replayed_from_a_captured_graph(g, device):
    pred, theta, kw = _nms_case("lds_cap")
    pd, td = pred.to(device), theta.to(device)
    eager = _run_nms(pd, td, kw, device)
    bufs = H.RNmsBuffers(pd.shape[0], pd.shape[2], 300, device)
    params = torch.tensor([[1.0, 0.0, 0.0, 640.0, 640.0]] * pd.shape[0], device=device)
    H.scale_rboxes_(eager, params)
    plan = H.LaunchPlan()
    with H.record(plan):
        _run_nms(pd, td, kw, device, bufs=bufs)
        H.scale_rboxes_(bufs, params)
    assert len(plan.ops) == 2
    torch.cuda.synchronize(device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        plan.replay(torch.cuda.current_stream().cuda_stream)
    for t in (bufs.out, bufs.index, bufs.count):
        t.fill_(3)
    graph.replay()
    torch.cuda.synchronize(device)
    assert torch.equal(bufs.count, eager.count) and torch.equal(bufs.index, eager.index) and torch.equal(bufs.out.view(torch.int32), eager.out.view(torch.int32))


# ---- dy_scale_rboxes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pad_x", "pad_y", "up"])
def test_scale_rboxes_against_construct_result(g, name, device):
    rows_in, exp = g[f"scale_{name}__in"], g[f"scale_{name}__out"]
    in_hw, orig_hw = (tuple(int(v) for v in r) for r in g[f"scale_{name}__shapes"])
    gain, px, py = ops.letterbox_params(in_hw, orig_hw)
    assert (px != 0) == (name == "pad_x") and (py != 0) == (name == "pad_y")
    k, max_det = len(rows_in), len(rows_in) + 4
    bufs = H.RNmsBuffers(2, 64, max_det, device)
    bufs.out.fill_(-3.0)
    bufs.out[0, :k] = torch.from_numpy(rows_in).to(device)
    bufs.out[1, : k - 5] = torch.from_numpy(rows_in[5:]).to(device)
    bufs.count.copy_(torch.tensor([k, k - 5], dtype=torch.int32))
    H.scale_rboxes_(bufs, torch.tensor([[gain, px, py, orig_hw[1], orig_hw[0]]] * 2, dtype=torch.float32, device=device))
    out = bufs.out.cpu().numpy()
    tol_th = float(g["dec_tol"][1])
    for got, ref in ((out[0, :k], exp), (out[1, : k - 5], exp[5:])):
        assert np.array_equal(got[:, :4], ref[:, :4]) and np.array_equal(got[:, 5:], ref[:, 5:])
        assert np.abs(got[:, 4] - ref[:, 4]).max() <= tol_th
    assert (out[0, k:] == -3.0).all() and (out[1, k - 5 :] == -3.0).all(), "rows behind the count must be untouched"
    assert exp[0, 2] == orig_hw[1] and exp[1, 2] == orig_hw[1], "the fixture's wide boxes are clamped to the image width (clip_boxes on xywh rows)"


# ---- end to end through YOLO(...).predict ----------------------------------------------------------------------------------------------
def _yolo(g, tag):
    m = meta(g, tag)
    y = YOLO(m["yaml"].replace("yolov8-", f"yolov8{m['scale']}-"))
    y.model = OBBModel(dict(load_yaml(m["yaml"], m["scale"], m["nc"])), nc=m["nc"], verbose=False)
    y.model.load_state_dict(O.seeded_state_dict(y.model.state_dict(), m["seed"], cls_bias=m["cls_bias"]))
    assert y.task == "obb"
    return y, m


def _xyxy(rows):
    return np.concatenate((rows[:, :2] - rows[:, 2:4] / 2, rows[:, :2] + rows[:, 2:4] / 2), 1)


def _theta_tol(g, tag):
    """The fixture's own angle bar: 8 x the difference between the reference's fp32 and float64 runs over all anchors of these inputs."""
    return float(meta(g, tag)["theta_tol"])


def _check(g, tag, res, y, what, bar=True):
    counts = [int(k) for k in g[f"{tag}__n"]]
    exp_rows, exp_idx = split_rows(g[f"{tag}__det"], counts), split_rows(g[f"{tag}__det_idx"], counts)
    cf = next(iter(y.predictor._compiled.values()))
    worst_iou, worst_th, kept = 1.0, 0.0, []
    for i, r in enumerate(res):
        assert r.boxes is None and r.obb is not None and r.obb.data.is_cuda and len(r) == len(r.obb) and r.obb.id is None
        rows = r.obb.data.cpu().numpy()
        kept.append(len(rows))
        if bar:
            assert len(rows) == counts[i], f"{what}: image {i} kept {len(rows)}, the reference {counts[i]}"
            assert np.array_equal(cf.nms.index[i, : counts[i]].cpu().numpy(), exp_idx[i]) and np.array_equal(rows[:, 6], exp_rows[i][:, 6])
        if len(rows) == counts[i] and counts[i]:
            worst_iou = min(worst_iou, float(box_iou_pairs(_xyxy(rows), _xyxy(exp_rows[i])).min()))
            worst_th = max(worst_th, float(np.abs(rows[:, 4] - exp_rows[i][:, 4]).max()))
            assert tuple(r.obb.xyxyxyxy.shape) == (counts[i], 4, 2) and tuple(r.obb.xyxy.shape) == (counts[i], 4)
    _report(what, {"kept": kept, "reference": counts, "min_iou_unrotated": worst_iou, "max_theta_err": worst_th, "theta_tol": _theta_tol(g, tag)})
    if bar:
        assert worst_iou >= 0.999 and worst_th <= _theta_tol(g, tag)


@pytest.mark.parametrize("dtype", ["fp32", None], ids=["f32", "split"])
@pytest.mark.parametrize("tag", ["obbn64x96", "obb3n64x96"])
def test_predict_rows_against_the_reference(g, tag, dtype, device):
    y, m = _yolo(g, tag)
    x = torch.rand(*m["shape"], generator=torch.Generator().manual_seed(m["seed"]))
    res = y.predict(x, device=0, dtype=dtype, conf=m["conf"], iou=m["iou"])
    assert y.predictor.dtype == (torch.float32 if dtype else X2) and type(y.predictor).__name__ == "OBBPredictor"
    _check(g, tag, res, y, f"predict {tag} {dtype or 'split'}")
    if dtype is None:
        streamed = list(y.predict(x, device=0, conf=m["conf"], iou=m["iou"], stream=True, batch=1))
        assert len(streamed) == len(res)
        for a, b in zip(streamed, res):
            assert torch.equal(a.obb.data, b.obb.data)
        y2, _ = _yolo(g, tag)  # half=True: measured, no bar (the 16-bit path runs in the scaled activation domain)
        _check(g, tag, y2.predict(x, device=0, half=True, conf=m["conf"], iou=m["iou"]), y2, f"predict {tag} half", bar=False)


@pytest.mark.parametrize("dtype", ["fp32", None], ids=["f32", "split"])
def test_predict_uint8_frame_through_the_letterbox(g, dtype, device):
    y, m = _yolo(g, "obbn_u8")
    frame = g["obbn_u8__frame"]
    res = y.predict([frame], device=0, dtype=dtype, conf=m["conf"], iou=m["iou"], imgsz=m["imgsz"])
    assert res[0].orig_shape == tuple(frame.shape[:2])
    _check(g, "obbn_u8", res, y, f"predict obbn_u8 {dtype or 'split'}")


def test_predict_arguments_act_as_for_detection(g, device):
    y, m = _yolo(g, "obbn64x96")
    x = torch.rand(*m["shape"], generator=torch.Generator().manual_seed(m["seed"]))
    full = y.predict(x, device=0, conf=m["conf"], iou=m["iou"])
    classes = sorted({int(c) for r in full for c in r.obb.cls.tolist()})[:1]
    only = y.predict(x, device=0, conf=m["conf"], iou=m["iou"], classes=classes)
    assert sum(len(r) for r in only) >= 1 and all(int(c) in classes for r in only for c in r.obb.cls.tolist())
    capped = y.predict(x, device=0, conf=m["conf"], iou=m["iou"], max_det=2)
    assert [len(r) for r in capped] == [min(len(r), 2) for r in full]
    for a, b in zip(capped, full):
        assert torch.equal(a.obb.data, b.obb.data[:2])
    none = y.predict(x, device=0, conf=0.999)
    assert all(len(r) == 0 and r.obb is not None and r.boxes is None for r in none)
    agn = y.predict(x, device=0, conf=m["conf"], iou=m["iou"], agnostic_nms=True)
    assert sum(len(r) for r in agn) <= sum(len(r) for r in full)
