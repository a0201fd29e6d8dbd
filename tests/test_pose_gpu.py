"""GPU parity of the pose path against tests/golden/pose.npz (tools/make_pose_golden.py: the REAL reference's Pose head, ``kpts_decode``,
``scale_coords`` + ``Keypoints`` and end-to-end predictions), and of the batched person-crop slicer against the whole-frame letterbox kernel.

Bars.  Head: ``RTOL[dtype]`` x the reference's scale, as tests/test_obb_gpu.py.  ``dy_kpt_decode``: x and y equal to the reference's fp32 arrays
bit for bit (every step of the expression is one rounded fp32 operation), the visibility within ``vis_tol`` = 8 x the reference's own
fp32-vs-float64 difference (the device's expf is not the CPU's); the gather form equal to the dense form bit for bit.  ``dy_scale_coords``:
equal to the recorded reference (subtraction, division and clamp are exact operations).  Slicer: equal to ``dy_letterbox_u8_to_nchw_f32`` on a
contiguous copy of each window, bit for bit.  End to end: kept anchors, classes and order exact, box IoU >= 0.999, keypoints within the fixture's
``kpt_tol`` (8 x the difference of the reference's fp32 and float64 runs) in fp32 and split float16, within ``RTOL[float16]`` x the image size
with ``half=True``.  ``predict(frames, crops=...)``: equal to the list-of-crops call plus the offset, bit for bit in fp32.
"""
import numpy as np
import pytest
import torch

from drone_yolo_amd import YOLO, _lib
from drone_yolo_amd import hip_ops as H
from drone_yolo_amd.engine import crops as CR
from drone_yolo_amd.nn import modules as M
from drone_yolo_amd.nn.tasks import PoseModel, initialize_weights
from oracle import drone_yolo_oracle as O
from oracle import letterbox_oracle as LB
from tests import _pose_util as U
from tests._util import box_iou_pairs, golden, load_yaml, meta, split_rows
from tests.test_model_gpu import RTOL as _RTOL
from tests.test_model_gpu import _report as _parity_report

pytestmark = pytest.mark.gpu
X2 = H.F16X2
RTOL = {**_RTOL, X2: _RTOL[torch.float32]}  # split float16 (22 mantissa bits) is held to fp32's


@pytest.fixture(scope="module")
def g():
    return golden("pose.npz")


def _report(name, payload):
    _parity_report(name, payload)
    print(name, payload)


# ---- head ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, X2, torch.float16, torch.bfloat16], ids=["f32", "split", "f16", "bf16"])
@pytest.mark.parametrize("name", ["a", "b"])
def test_head_matches_reference_vectors(g, name, dtype, device):
    spec = U.HEADS[name]
    nc, nk = spec["nc"], spec["kpt_shape"][0] * spec["kpt_shape"][1]
    M.Pose.legacy = True
    head = M.Pose(nc=nc, kpt_shape=spec["kpt_shape"], ch=U.HEAD_CH)
    head.load_state_dict(O.seeded_state_dict(head.state_dict(), int(g[f"head_{name}_seed"])))
    initialize_weights(head)
    head = head.to(device).eval()
    head.stride = torch.tensor(U.HEAD_STRIDES)
    s = int(g[f"head_{name}_xseed"])
    xs = [H.to_nhwc(U.randn(s + i, *shape).to(device), dtype) for i, shape in enumerate(U.HEAD_MAPS)]
    y, (feats, kpt) = head(xs)
    assert tuple(y.shape) == (2, 4 + nc + nk, 120) and tuple(kpt.shape) == (2, nk, 120) and len(feats) == 2
    for what, got, ref in (("Pose y", y[:, : 4 + nc], g[f"head_{name}_y"]), ("Pose kpt", kpt, g[f"head_{name}_kpt"]), ("Pose pred_kpt", y[:, 4 + nc :], g[f"head_{name}_pred_kpt"])):
        ref = torch.from_numpy(ref)
        err, scale = float((got.float().cpu() - ref).abs().max()), float(ref.abs().max())
        _report(f"{what} {name}", {"dtype": str(dtype), "max_abs_err": err, "scale": scale})
        assert err <= RTOL[dtype] * scale, f"{what} {name} [{dtype}]: max|err| {err:.4e}, scale {scale:.3f}"
    head.fuse_tail = True  # the predictor's form: nothing concatenated
    try:
        y2, (none, levels) = head(xs)
    finally:
        head.fuse_tail = False
    assert none is None and tuple(y2.shape) == (2, 4 + nc, 120) and torch.equal(y2, y[:, : 4 + nc])
    assert [tuple(l.shape) for l in levels] == [(2, nk, 8, 12), (2, nk, 4, 6)] and all(l.dtype == torch.float32 for l in levels)
    assert torch.equal(torch.cat([l.reshape(2, nk, -1) for l in levels], 2), kpt)
    assert torch.equal(H.kpt_decode(levels, U.HEAD_STRIDES, spec["kpt_shape"]), y[:, 4 + nc :])
    maps = head.keypoint_maps(xs)
    assert all(torch.equal(a, b) for a, b in zip(maps, levels))
    head.train()
    with pytest.raises(NotImplementedError):
        head(xs)


# ---- dy_kpt_decode ----------------------------------------------------------------------------------------------------------------
def _dense(g, name, device):
    kpt_shape = U.DECODE_SHAPES[name]
    levels = U.padded_levels(U.decode_logits(int(g[f"{name}_seed"]), kpt_shape), device)
    strides = [s for _, _, s in U.DECODE_LEVELS]
    return kpt_shape, levels, strides, H.kpt_decode(levels, strides, kpt_shape)


@pytest.mark.parametrize("name", list(U.DECODE_SHAPES))
def test_kpt_decode_dense_against_the_reference(g, name, device):
    kpt_shape, levels, strides, out = _dense(g, name, device)
    ref = g[f"{name}_ref32"]
    got = out.cpu().numpy()
    assert got.shape == ref.shape == (U.DECODE_BATCH, kpt_shape[0] * kpt_shape[1], sum(h * w for h, w, _ in U.DECODE_LEVELS))
    nd = kpt_shape[1]
    assert np.array_equal(got[:, 0::nd], ref[:, 0::nd]) and np.array_equal(got[:, 1::nd], ref[:, 1::nd]), "x and y must equal the reference's fp32 arrays bit for bit"
    if nd == 3:
        tol = float(g[f"{name}_vis_tol"])
        err = float(np.abs(got[:, 2::3].astype(np.float64) - g[f"{name}_ref64"][:, 2::3]).max())
        _report(f"dy_kpt_decode {name}", {"max_err_vis": err, "vis_tol": tol})
        assert err <= tol
        last = U.DECODE_LEVELS[0][0] * U.DECODE_LEVELS[0][1] - 1  # the saturated logits (-40, 40; 90, -90) of the first level's first and last anchor
        assert float(got[0, 2, 0]) <= tol and float(got[1, 2, 0]) == 1.0 and float(got[0, 2, last]) == 1.0 and float(got[1, 2, last]) == 0.0
        assert np.isfinite(got).all()


def test_kpt_decode_refuses_what_is_not_built(device):
    lv = [torch.zeros((1, 4, 4, 1024), device=device).permute(0, 3, 1, 2)]
    with pytest.raises(_lib.DyoloError):
        H.kpt_decode([lv[0][:, :16]], [8.0], (4, 4))
    with pytest.raises(_lib.DyoloError):
        H.kpt_decode([lv[0][:, :4]], [8.0], (4, 1))
    with pytest.raises(_lib.DyoloError):
        H.kpt_decode([lv[0][:, :258]], [8.0], (86, 3))  # nk = 258 > 256
    assert tuple(H.kpt_decode([lv[0][:, :255]], [8.0], (85, 3)).shape) == (1, 255, 16)


@pytest.mark.parametrize("name", list(U.DECODE_SHAPES))
def test_kpt_decode_gather_equals_dense_at_the_kept_anchors(g, name, device):
    kpt_shape, levels, strides, dense = _dense(g, name, device)
    nk, A = dense.shape[1], dense.shape[2]
    max_det = 8
    levels = [torch.cat([l, l[:1]], 0) for l in levels]  # a third image: a copy of the first
    levels = [H.alloc_nhwc(3, nk, l.shape[2], l.shape[3], torch.float32, device, ld=nk + 3).copy_(l) for l in levels]
    bufs = H.NmsBuffers(3, A, max_det, device)
    index = torch.tensor([[5, 4, 3, 2, 1, 0, 6, 7], [A - 1, 0, 35, 34, 36, 1, 20, A - 2], [A - 1, -1, A, 0, 2 ** 30, 7, 7, 7]], dtype=torch.int32)
    bufs.index.copy_(index)
    bufs.count.copy_(torch.tensor([0, max_det, 5], dtype=torch.int32))  # none, a full max_det, and rows with indices outside [0, A)
    out = torch.full((3, max_det, nk), -7.0, dtype=torch.float32, device=device)
    assert H.kpt_gather(bufs, levels, strides, kpt_shape, out=out).data_ptr() == out.data_ptr()
    got, dn = out.cpu(), dense.cpu()
    assert bool((got[0] == -7.0).all()), "an image without detections must be left untouched"
    assert torch.equal(got[1].view(torch.int32), dn[1][:, index[1].long()].t().contiguous().view(torch.int32))
    assert torch.equal(got[2, 0].view(torch.int32), dn[0][:, A - 1].contiguous().view(torch.int32)) and torch.equal(got[2, 3], dn[0][:, 0])
    assert bool((got[2, [1, 2, 4]] == 0).all()), "an index outside [0, anchors) writes zeros"
    assert bool((got[2, 5:] == -7.0).all()), "rows behind the count must be untouched"
    with pytest.raises(ValueError):
        H.kpt_gather(H.NmsBuffers(3, A + 1, max_det, device), levels, strides, kpt_shape)


# ---- dy_scale_coords --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(U.SCALE_CASES))
def test_scale_coords_against_the_reference(g, name, device):
    in_hw, orig_hw = U.SCALE_CASES[name]
    kp = U.scale_inputs(int(g[f"sc_{name}_seed"]), in_hw)
    exp = g[f"sc_{name}_out"]
    n, nkpt, nd = kp.shape
    max_det = n + 3
    gain = min(in_hw[0] / orig_hw[0], in_hw[1] / orig_hw[1])
    pad = ((in_hw[1] - orig_hw[1] * gain) / 2, (in_hw[0] - orig_hw[0] * gain) / 2)
    off = (37.0, 1021.0)
    rows = torch.full((3, max_det, nkpt * nd), -3.0, dtype=torch.float32, device=device)
    rows[0, :n], rows[1, : n - 2], rows[2, :n] = kp.view(n, -1).to(device), kp[2:].view(n - 2, -1).to(device), kp.view(n, -1).to(device)
    count = torch.tensor([n, n - 2, 0], dtype=torch.int32, device=device)
    params = torch.tensor([[gain, *pad, orig_hw[1], orig_hw[0], 0.0, 0.0], [gain, *pad, orig_hw[1], orig_hw[0], *off], [gain, *pad, orig_hw[1], orig_hw[0], *off]],
                          dtype=torch.float32, device=device)
    boxes = torch.arange(3 * max_det * 6, dtype=torch.float32, device=device).view(3, max_det, 6)
    boxes0 = boxes.cpu().clone()
    H.scale_coords_(rows, count, params, (nkpt, nd), boxes=boxes)
    out, bx = rows.cpu().numpy(), boxes.cpu()
    assert np.array_equal(out[0, :n].reshape(n, nkpt, nd), exp), "scale_coords + Keypoints masking must equal the reference bit for bit"
    shifted = exp[2:].copy()
    vis = shifted[..., 2] >= 0.5
    shifted[..., 0][vis] += np.float32(off[0])
    shifted[..., 1][vis] += np.float32(off[1])
    assert bool((~vis).any()) and np.array_equal(out[1, : n - 2].reshape(n - 2, nkpt, nd), shifted), "visible points take the offset, invisible ones stay at (0, 0)"
    assert (out[0, n:] == -3.0).all() and (out[1, n - 2 :] == -3.0).all() and (out[2, n:] == -3.0).all(), "rows behind the count must be untouched"
    assert np.array_equal(out[2, :n], kp.view(n, -1).numpy()), "an image whose count is 0 must be left as it is"
    assert torch.equal(bx[0], boxes0[0]) and torch.equal(bx[2], boxes0[2]) and torch.equal(bx[1, n - 2 :], boxes0[1, n - 2 :])
    assert torch.equal(bx[1, : n - 2], boxes0[1, : n - 2] + torch.tensor([off[0], off[1], off[0], off[1], 0.0, 0.0]))


# ---- the crop slicer --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("imgsz", [64, 66], ids=["vector", "scalar"])
def test_crop_slicer_equals_the_letterbox_of_each_window(imgsz, device):
    frames = U.crop_frames()
    rects = CR.crop_rects(list(frames), U.CROP_BOXES, U.CROP_EXPAND)
    table = torch.from_numpy(CR.crop_table(rects, imgsz))
    fd = torch.from_numpy(frames).to(device)
    guard = 64
    flat = torch.full((5 * 3 * imgsz * imgsz + 2 * guard,), -5.0, dtype=torch.float32, device=device)
    out = flat[guard:-guard].view(5, 3, imgsz, imgsz)
    H.crops_letterbox(fd, table, imgsz, imgsz, out=out)
    assert bool((flat[:guard] == -5.0).all()) and bool((flat[-guard:] == -5.0).all()), "the slicer wrote outside its output"
    for j, (f, x0, y0, x1, y1) in enumerate(rects):
        win = torch.from_numpy(np.ascontiguousarray(frames[f, y0:y1, x0:x1])).to(device)
        _, _, _, cw, ch, nw, nh, top, left = table[j].tolist()
        ref = H.letterbox(win[None], nw, nh, top, left, imgsz, imgsz, True)
        assert torch.equal(out[j].view(torch.int32), ref[0].view(torch.int32)), f"crop {j} ({cw}x{ch} -> {nw}x{nh}) differs from the letterbox of its window"
        host = LB.preprocess([frames[f, y0:y1, x0:x1]], imgsz=(imgsz, imgsz), auto=False)[0]
        assert np.array_equal(out[j].cpu().numpy(), host), f"crop {j} differs from the letterbox oracle"
    one = H.crops_letterbox(fd, table[3:4].contiguous(), imgsz, imgsz)  # a single crop
    assert torch.equal(one[0], out[3])


@pytest.mark.parametrize("bad", [(0, 100, 0, 41, 10), (0, -1, 0, 10, 10), (0, 0, 85, 10, 6), (2, 0, 0, 10, 10), (0, 5, 5, 0, 10), (0, 5, 5, 10, 0)],
                         ids=["right", "left", "bottom", "frame", "cw0", "ch0"])
def test_crop_slicer_refuses_a_bad_table_row_without_a_launch(bad, device):
    frames = U.crop_frames()
    rects = CR.crop_rects(list(frames), U.CROP_BOXES, U.CROP_EXPAND)
    table = torch.from_numpy(CR.crop_table(rects, 64))
    f, x0, y0, cw, ch = bad
    table[2, :5] = torch.tensor([f, x0, y0, cw, ch], dtype=torch.int32)
    out = torch.full((5, 3, 64, 64), -5.0, dtype=torch.float32, device=device)
    with pytest.raises(_lib.DyoloError, match="crop 2"):
        H.crops_letterbox(torch.from_numpy(frames).to(device), table, 64, 64, out=out)
    torch.cuda.synchronize(device)
    assert bool((out == -5.0).all()), "nothing may be launched for a table with a bad row"


# ---- end to end through YOLO(...).predict ----------------------------------------------------------------------------------------------
def _yolo(g, tag):
    m = meta(g, tag)
    y = YOLO(m["yaml"].replace("yolov8-", f"yolov8{m['scale']}-"))
    y.model = PoseModel(dict(load_yaml(m["yaml"], m["scale"], m["nc"])), nc=m["nc"], verbose=False)
    y.model.load_state_dict(O.seeded_state_dict(y.model.state_dict(), m["seed"], cls_bias=m["cls_bias"]))
    assert y.task == "pose"
    return y, m


def _check(g, tag, res, y, what, xy_tol, vis_tol):
    m = meta(g, tag)
    counts = [int(k) for k in g[f"{tag}__n"]]
    exp_rows, exp_idx, exp_kp = split_rows(g[f"{tag}__det"], counts), split_rows(g[f"{tag}__det_idx"], counts), split_rows(g[f"{tag}__kpts"], counts)
    cf = next(iter(y.predictor._compiled.values()))
    kept = [len(r) for r in res]
    worst_iou, worst_xy, worst_vis = 1.0, 0.0, 0.0
    same = kept == counts and all(np.array_equal(cf.nms.index[i, :k].cpu().numpy(), exp_idx[i]) for i, k in enumerate(counts))
    if same:
        for i, r in enumerate(res):
            assert r.boxes is not None and r.keypoints is not None and r.keypoints.data.is_cuda and r.keypoints.data.dtype == torch.float32
            assert tuple(r.keypoints.data.shape) == (counts[i], *m["kpt_shape"]) and len(r) == counts[i] and r.keypoints.has_visible
            if not counts[i]:
                continue
            rows, kp = r.boxes.data.cpu().numpy(), r.keypoints.data.cpu().numpy()
            worst_iou = min(worst_iou, float(box_iou_pairs(rows[:, :4], exp_rows[i][:, :4]).min()))
            worst_xy = max(worst_xy, float(np.abs(kp[..., :2].astype(np.float64) - exp_kp[i][..., :2]).max()))
            worst_vis = max(worst_vis, float(np.abs(kp[..., 2].astype(np.float64) - exp_kp[i][..., 2]).max()))
    _report(what, {"kept": kept, "reference": counts, "same_anchors": same, "min_iou": worst_iou, "max_xy_err": worst_xy, "xy_tol": xy_tol, "max_vis_err": worst_vis,
                   "vis_tol": vis_tol})
    assert same, f"{what}: kept {kept}, the reference {counts} (or other anchors / another order)"
    for i, r in enumerate(res):
        assert np.array_equal(r.boxes.cls.cpu().numpy(), exp_rows[i][:, 5])
    assert worst_iou >= 0.999 and worst_xy <= xy_tol and worst_vis <= vis_tol


@pytest.mark.parametrize("dtype", ["fp32", None], ids=["f32", "split"])
@pytest.mark.parametrize("tag", ["pose3n64x96", "posen64x96"])
def test_predict_rows_against_the_reference(g, tag, dtype, device):
    y, m = _yolo(g, tag)
    x = torch.rand(*m["shape"], generator=torch.Generator().manual_seed(m["seed"]))
    res = y.predict(x, device=0, dtype=dtype, conf=m["conf"], iou=m["iou"])
    assert y.predictor.dtype == (torch.float32 if dtype else X2) and type(y.predictor).__name__ == "PosePredictor"
    _check(g, tag, res, y, f"predict {tag} {dtype or 'split'}", m["kpt_tol"], m["vis_tol"])
    if dtype is None:
        streamed = list(y.predict(x, device=0, conf=m["conf"], iou=m["iou"], stream=True, batch=1))
        assert len(streamed) == len(res)
        for a, b in zip(streamed, res):
            assert torch.equal(a.boxes.data, b.boxes.data) and torch.equal(a.keypoints.data, b.keypoints.data)


@pytest.mark.parametrize("tag", ["pose3n64x96", "posen64x96"])
def test_predict_half_against_the_reference(g, tag, device):
    y, m = _yolo(g, tag)
    x = torch.rand(*m["shape"], generator=torch.Generator().manual_seed(m["seed"]))
    res = y.predict(x, device=0, half=True, conf=m["conf"], iou=m["iou"])
    assert y.predictor.dtype == torch.float16
    _check(g, tag, res, y, f"predict {tag} half", RTOL[torch.float16] * max(m["shape"][2:]), RTOL[torch.float16])


@pytest.mark.parametrize("dtype", ["fp32", None, "half"], ids=["f32", "split", "half"])
def test_predict_uint8_frame_through_the_letterbox(g, dtype, device):
    y, m = _yolo(g, "posen_u8")
    frame = g["posen_u8__frame"]
    kw = dict(half=True) if dtype == "half" else dict(dtype=dtype)
    res = y.predict([frame], device=0, conf=m["conf"], iou=m["iou"], imgsz=m["imgsz"], **kw)
    assert res[0].orig_shape == tuple(frame.shape[:2]) and res[0].crop is None
    assert y.predictor.dtype == {"fp32": torch.float32, None: X2, "half": torch.float16}[dtype]
    tol = (RTOL[torch.float16] * max(frame.shape[:2]), RTOL[torch.float16]) if dtype == "half" else (m["kpt_tol"], m["vis_tol"])
    _check(g, "posen_u8", res, y, f"predict posen_u8 {dtype or 'split'}", *tol)
    kp = res[0].keypoints
    assert tuple(kp.xy.shape) == (len(res[0]), 17, 2) and tuple(kp.conf.shape) == (len(res[0]), 17)
    assert bool((kp.xyn <= 1).all()) and bool((kp.xy[kp.conf < 0.5] == 0).all())


# ---- predict(frames, crops=...) -----------------------------------------------------------------------------------------------------------
def test_predict_crops_equals_the_list_of_crops_plus_the_offset(g, device):
    y, m = _yolo(g, "posen_u8")
    frames = U.crop_frames()
    rects = U.CROP_RECTS
    kw = dict(device=0, dtype="fp32", conf=0.05, iou=m["iou"], imgsz=64, batch=2)
    # the last batch of the list call holds ONE crop, which the predictor letterboxes to its minimum rectangle: for this crop that is the same geometry
    last = rects[-1]
    assert LB.letterbox_geometry((last[4] - last[2], last[3] - last[1]), (64, 64), auto=True) == LB.letterbox_geometry((last[4] - last[2], last[3] - last[1]), (64, 64), auto=False)
    res = y.predict(frames, crops=U.CROP_BOXES, crop_expand=U.CROP_EXPAND, **kw)
    assert type(y.predictor).__name__ == "PosePredictor" and len(res) == 5
    y2, _ = _yolo(g, "posen_u8")
    ref = y2.predict([np.ascontiguousarray(frames[f, y0:y1, x0:x1]) for f, x0, y0, x1, y1 in rects], **kw)
    assert len(ref) == 5 and sum(len(r) for r in ref) >= 3, "the case must detect something"
    for r, q, rect in zip(res, ref, rects):
        f, x0, y0, x1, y1 = rect
        assert r.crop == rect and r.orig_shape == tuple(frames.shape[1:3]) and q.orig_shape == (y1 - y0, x1 - x0) and len(r) == len(q)
        off = torch.tensor([x0, y0, x0, y0, 0, 0], dtype=torch.float32)
        assert torch.equal(r.boxes.data.cpu().view(torch.int32), (q.boxes.data.cpu() + off).view(torch.int32))
        exp = q.keypoints.data.cpu().clone()
        vis = exp[..., 2] >= 0.5
        exp[..., 0][vis] += float(x0)
        exp[..., 1][vis] += float(y0)
        assert torch.equal(r.keypoints.data.cpu(), exp), "keypoints of a crop = keypoints of the list call + the crop's offset, invisible ones at (0, 0)"
        if len(r):
            b = r.boxes.data.cpu()
            assert bool((b[:, 0] >= x0).all()) and bool((b[:, 2] <= x1).all()) and bool((b[:, 1] >= y0).all()) and bool((b[:, 3] <= y1).all())
    streamed = list(y.predict(frames, crops=U.CROP_BOXES, crop_expand=U.CROP_EXPAND, stream=True, **kw))
    assert all(torch.equal(a.keypoints.data, b.keypoints.data) and torch.equal(a.boxes.data, b.boxes.data) for a, b in zip(streamed, res))
