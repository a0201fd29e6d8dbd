"""GPU parity of the segmentation path against tests/golden/seg.npz (tools/make_seg_golden.py: the REAL reference's modules, mask
functions and end-to-end predictions): Proto / Segment / the transposed convolution in every storage type, ``dy_process_mask`` on the
mask-assembly cases, ``dy_mask_gather`` in both forms, and ``YOLO(...).predict`` end to end.

Mask bars.  Kernel level: equal to the reference's mask on every pixel outside the fixture's UNSURE bitmap (|v| below the worst-case fp32
rounding of the 32-term dot product and the blend, see the tool).  End to end the prototypes and coefficients themselves carry the
network's rounding, so the bar is a count of differing pixels: at most 4x (fp32: another ordering of the same sums — its distance to the
CPU fp32 result is at most the two distances to exact, times 2 of headroom) or 16x (split float16: stored activations carry 22 bits) the
share on which the reference's own float64 and fp32 runs differ, with a floor of 2 pixels per detection; a shifted crop edge or a
half-pixel error moves a full row of >= 8 pixels.  The differing pixels are counted over the WHOLE masks (not only inside the boxes),
which asks no less.
"""
import numpy as np
import pytest
import torch

import drone_yolo_amd as D
from drone_yolo_amd import YOLO
from drone_yolo_amd import hip_ops as H
from drone_yolo_amd.nn import modules as M
from drone_yolo_amd.nn.tasks import SegmentationModel, initialize_weights
from oracle import drone_yolo_oracle as O
from tests._util import box_iou_pairs, golden, load_yaml, meta, split_rows
from tests.test_model_gpu import RTOL as _RTOL
from tests.test_model_gpu import _report as _parity_report

pytestmark = pytest.mark.gpu
X2 = H.F16X2
# module-vector tolerances per storage type: tests/test_model_gpu.py's; split float16 (22 mantissa bits, not listed there) takes fp32's
RTOL = {**_RTOL, X2: _RTOL[torch.float32]}
DTYPES = [torch.float32, torch.float16, torch.bfloat16, X2]
IDS = ["f32", "f16", "bf16", "split"]
NM = 32


@pytest.fixture(scope="module")
def g():
    return golden("seg.npz")


def _report(name, payload):
    """The measured figure into the suite's parity report (tests/test_model_gpu.py::_report) and onto stdout (``pytest -s``)."""
    _parity_report(name, payload)
    print(name, payload)


def _randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _dev(t, dtype, device):
    return H.to_nhwc(t.to(device).contiguous(), dtype)


def _f32(t):
    return (t.float() if t.dtype == torch.float32 else H.to_nchw_f32(t)).cpu()


def _close(got, ref, dtype, what):
    scale = float(ref.abs().max())
    err = float((_f32(got) - ref).abs().max())
    _report(what, {"dtype": str(dtype), "max_abs_err": err, "scale": scale})
    assert err <= RTOL[dtype] * scale, f"{what} [{dtype}]: max|err| {err:.4e}, scale {scale:.3f}"


def _seeded(mod, seed, device):
    mod.load_state_dict(O.seeded_state_dict(mod.state_dict(), seed))
    initialize_weights(mod)
    return mod.to(device).eval()


# ---- module vectors -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_modules_match_reference_vectors(g, dtype, device):
    t = lambda k: torch.from_numpy(g[k])  # noqa: E731
    # ConvTranspose2d(32, 32, 2, 2): the 1x1 GEMM on the repacked weights + dy_depth_to_space2_nhwc
    ct = torch.nn.ConvTranspose2d(32, 32, 2, 2, 0, bias=True)
    ct.load_state_dict(O.seeded_state_dict(ct.state_dict(), int(g["deconv_seed"])))
    pc = H.PackedConv(*H.deconv2x2_as_conv1x1(ct.weight, ct.bias), 1, 0, 1, False, dtype, device)
    y = H.conv_transpose2x2(_dev(_randn(int(g["deconv_xseed"]), 2, 32, 5, 7), dtype, device), pc)
    assert tuple(y.shape) == (2, 32, 10, 14) and y.dtype == dtype
    _close(y, t("deconv_y"), dtype, "ConvTranspose2d k2 s2")
    proto = _seeded(M.Proto(32, 64, 32), int(g["proto_seed"]), device)
    p = proto(_dev(_randn(int(g["proto_xseed"]), 2, 32, 12, 20), dtype, device))
    assert p.dtype == torch.float32 and tuple(p.shape) == (2, 32, 24, 40) and H.view_params(p)[1] == 32  # fp32 NHWC whatever the storage type
    _close(p, t("proto_y"), dtype, "Proto")
    M.Segment.legacy = True
    head = M.Segment(nc=10, nm=32, npr=64, ch=(32, 64))
    head = _seeded(head, int(g["seghead_seed"]), device)
    head.stride = torch.tensor([8.0, 16.0])
    xs = [_dev(_randn(int(g["seghead_xseed"]), 1, 32, 12, 20), dtype, device), _dev(_randn(int(g["seghead_xseed"]) + 1, 1, 64, 6, 10), dtype, device)]
    y, (feats, mc, p) = head(xs)
    assert tuple(y.shape) == (1, 4 + 10 + 32, 300) and len(feats) == 2 and torch.equal(y[:, 14:], mc)
    _close(mc, t("seghead_mc"), dtype, "Segment mc")
    _close(p, t("seghead_p"), dtype, "Segment p")
    if dtype in (torch.float32, X2):
        assert torch.allclose(y[:, :14].cpu(), t("seghead_y"), rtol=1e-4, atol=5e-3)
    # the predictor's form: Detect's output alone, the coefficients as per-level fp32 NHWC maps, nothing concatenated
    head.fuse_tail = True
    try:
        y2, (none, levels, p2) = head(xs)
    finally:
        head.fuse_tail = False
    assert none is None and tuple(y2.shape) == (1, 14, 300) and [tuple(l.shape) for l in levels] == [(1, 32, 12, 20), (1, 32, 6, 10)]
    assert all(l.dtype == torch.float32 and H.view_params(l)[1] == 32 for l in levels)
    assert torch.equal(torch.cat([l.reshape(1, 32, -1) for l in levels], 2), mc) and torch.equal(p2, p)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_protos_and_coefficients_leave_the_scaled_domain_in_true_units(g, dtype, device):
    """In a pass whose stored activations are log2(e) times the reference's, Proto.cv3 and cv4's last conv hand out TRUE units."""
    t = lambda k: torch.from_numpy(g[k])  # noqa: E731
    proto = _seeded(M.Proto(32, 64, 32), int(g["proto_seed"]), device)
    M.Segment.legacy = True
    head = _seeded(M.Segment(nc=10, nm=32, npr=64, ch=(32, 64)), int(g["seghead_seed"]), device)
    s = int(g["seghead_xseed"])
    with H.scaled_activations(True):
        p = proto(_dev(_randn(int(g["proto_xseed"]), 2, 32, 12, 20) * H.LOG2E, dtype, device))
        levels = head.coefficient_maps([_dev(_randn(s, 1, 32, 12, 20) * H.LOG2E, dtype, device), _dev(_randn(s + 1, 1, 64, 6, 10) * H.LOG2E, dtype, device)])
    _close(p, t("proto_y"), dtype, "Proto (scaled domain)")
    _close(torch.cat([l.reshape(1, 32, -1) for l in levels], 2), t("seghead_mc"), dtype, "Segment mc (scaled domain)")


# ---- dy_depth_to_space2_nhwc: a pure permutation, checked bit for bit on a strided view ------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["2byte", "4byte"])
def test_depth_to_space_is_the_exact_permutation(dtype, device):
    n, c, h, w = 3, 24, 5, 7  # odd sizes, more than one workgroup
    buf = H.alloc_nhwc(n, 4 * c + 16, h, w, dtype, device)  # the source is a channel slice of a wider buffer (ld_x > 4c)
    buf.copy_(torch.randn(buf.shape, device=device).to(dtype))
    x = buf[:, 8 : 8 + 4 * c]
    out = H.alloc_nhwc(n, c + 8, 2 * h, 2 * w, dtype, device)[:, :c]
    y = H.depth_to_space2(x, out=out)
    ref = x.reshape(n, 2, 2, c, h, w).permute(0, 3, 4, 1, 5, 2).reshape(n, c, 2 * h, 2 * w)
    assert torch.equal(y, ref)
    with pytest.raises(H._lib.DyoloError):
        H.depth_to_space2(H.alloc_nhwc(1, 48, 2, 2, torch.float32, device))  # c = 12: not whole groups of 8


# ---- dy_process_mask on the mask-assembly cases -----------------------------------------------------------------------------------------
def _unpack(bits, shape):
    return np.unpackbits(bits)[: int(np.prod(shape))].reshape(shape).astype(bool)


@pytest.mark.parametrize("tag", ["pm_r4", "pm_r2", "pm_retina", "pm_win"])
def test_process_mask_cases(g, tag, device):
    m = meta(g, tag)
    counts = [int(k) for k in g[f"{tag}__counts"]]
    n, md, T = len(counts), m["max_det"], sum(counts)
    oh, ow = m["out_hw"]
    protos = _randn(m["seed"], n, m["mh"], m["mw"], NM).to(device)  # NHWC memory
    coef = _randn(m["seed"] + 1, n, md, NM)
    boxes = torch.from_numpy(g[f"{tag}__boxes"])
    side = torch.cat([boxes, coef], 2)
    rows = torch.cat([boxes, torch.zeros(n, md, 2)], 2)
    for b, k in enumerate(counts):  # rows beyond the counts must never be read: poison them
        side[b, k:] = float("nan")
        rows[b, k:] = float("nan")
    side, rows = side.to(device).contiguous(), rows.to(device).contiguous()
    count = torch.tensor(counts, dtype=torch.int32, device=device)
    pv = protos.permute(0, 3, 1, 2)
    if m["mode"] == "default":
        got = H.process_mask(pv, side, count, counts, (oh, ow), ratio=(m["mw"] / m["in_hw"][1], m["mh"] / m["in_hw"][0]))
    else:
        got = H.process_mask(pv, side, count, counts, (oh, ow), windows=g[f"{tag}__windows"].tolist(), crop_rows=rows)
    torch.cuda.synchronize()
    assert got.dtype == torch.uint8 and tuple(got.shape) == (T, oh, ow) and int(got.max()) <= 1
    got = got.cpu().numpy().astype(bool)
    ref, unsure, inbox = (_unpack(g[f"{tag}__{k}"], (T, oh, ow)) for k in ("masks", "unsure", "inbox"))
    share = float((unsure & inbox).sum()) / max(int(inbox.sum()), 1)
    wrong = int(((got != ref) & ~unsure).sum())
    _report(f"process_mask {tag}", {"masks": T, "pixels": int(ref.size), "set": int(ref.sum()), "unsure_share": share, "differ_in_unsure": int(((got != ref) & unsure).sum()), "wrong": wrong})
    assert ref.sum() > 0 and share <= 1e-3
    assert wrong == 0, f"{tag}: {wrong} pixels differ from the reference outside the unsure set"
    if tag == "pm_r4":
        assert counts == [5, 0, 8] and not got[5 + 4].any()  # an image without detections in the middle; the box narrower than a proto pixel
    # no detections at all: an empty tensor, nothing launched
    none = H.process_mask(pv, side, torch.zeros_like(count), [0] * n, (oh, ow))
    assert tuple(none.shape) == (0, oh, ow)


def test_mask_gather_forms_agree(device):
    n, nc, md = 3, 5, 8
    hw = [(12, 20), (6, 10)]
    A = sum(h * w for h, w in hw)
    gen = torch.Generator().manual_seed(3)
    pred = torch.zeros(n, 4 + nc + NM, A)
    pred[:, 0] = torch.rand(n, A, generator=gen) * 600 + 20
    pred[:, 1] = torch.rand(n, A, generator=gen) * 400 + 20
    pred[:, 2:4] = torch.rand(n, 2, A, generator=gen) * 60 + 10
    pred[:, 4 : 4 + nc] = torch.rand(n, nc, A, generator=gen) * 0.2
    hot = torch.randperm(A, generator=gen)
    pred[0, 4, hot[:40]] = 0.9  # image 0: more candidates than max_det; image 1: three; image 2: none
    pred[1, 6, hot[40:43]] = 0.8
    pred[:, 4 + nc :] = torch.randn(n, NM, A, generator=gen)
    pred = pred.to(device).contiguous()
    bufs = H.nms(pred, 0.5, 0.7, max_det=md, nc=nc)
    torch.cuda.synchronize()
    counts = bufs.count.tolist()
    assert counts[0] == md and 0 < counts[1] <= 3 and counts[2] == 0
    sentinel = torch.full((n, md, 4 + NM), -7.0, device=device)
    a = H.mask_gather(bufs, pred=pred, nc=nc, out=sentinel.clone())
    levels, a0 = [], 0
    for h, w in hw:  # the same coefficients as per-level NHWC maps, pitch above nm on the first level
        buf = H.alloc_nhwc(n, NM + 4, h, w, torch.float32, device)[:, :NM]
        buf.copy_(pred[:, 4 + nc :, a0 : a0 + h * w].reshape(n, NM, h, w))
        levels.append(buf)
        a0 += h * w
    b = H.mask_gather(bufs, levels=levels, out=sentinel.clone())
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    for i, k in enumerate(counts):
        idx = bufs.index[i, :k].long()
        assert torch.equal(a[i, :k, :4], bufs.out[i, :k, :4]) and torch.equal(a[i, :k, 4:], pred[i, 4 + nc :, idx].T)
        assert bool((a[i, k:] == -7.0).all())  # rows beyond the count: untouched


# ---- end to end through YOLO(...).predict ----------------------------------------------------------------------------------------------
def _yolo(g, tag):
    m = meta(g, tag)
    y = YOLO(m["yaml"].replace("yolov8-", f"yolov8{m['scale']}-"))
    y.model = SegmentationModel(dict(load_yaml(m["yaml"], m["scale"], m["nc"])), nc=m["nc"], verbose=False)
    y.model.load_state_dict(O.seeded_state_dict(y.model.state_dict(), m["seed"], cls_bias=m["cls_bias"]))
    assert y.task == "segment"
    return y, m


def _check(g, tag, sfx, res, y, mult, what, bar=True):
    counts = [int(k) for k in g[f"{tag}__n"]]
    exp_rows = split_rows(g[f"{tag}{sfx}__det"], counts)
    exp_idx = split_rows(g[f"{tag}__det_idx"], counts)
    T = sum(counts)
    hw = next(tuple(r.masks.shape[1:]) for r in res if r.masks is not None)
    ref = split_rows(_unpack(g[f"{tag}{sfx}__masks"], (T, *hw)), counts)
    share, inbox, _ = (float(v) for v in g[f"{tag}{sfx}__share64"])
    cf = next(iter(y.predictor._compiled.values()))
    differ = 0
    for i, r in enumerate(res):
        rows = r.boxes.data.cpu().numpy()
        if bar:
            assert len(rows) == counts[i], f"{what}: image {i} kept {len(rows)}, the reference {counts[i]}"
            assert np.array_equal(cf.nms.index[i, : counts[i]].cpu().numpy(), exp_idx[i]) and np.array_equal(rows[:, 5], exp_rows[i][:, 5])
            assert box_iou_pairs(rows[:, :4], exp_rows[i][:, :4]).min() >= 0.999
        if len(rows) == counts[i] and counts[i]:
            assert r.masks.data.dtype == torch.uint8 and r.masks.data.is_cuda and tuple(r.masks.shape) == (counts[i], *hw) and r.masks.orig_shape == r.orig_shape
            differ += int((r.masks.data.cpu().numpy().astype(bool) != ref[i]).sum())
    limit = max(mult * share * inbox, 2.0 * T)
    _report(what, {"differing_pixels": differ, "in_box_pixels": inbox, "share": differ / max(inbox, 1), "fixture_f64_share": share, "limit_pixels": limit, "detections": T})
    if bar:
        assert differ <= limit, f"{what}: {differ} mask pixels differ from the reference's, limit {limit}"


@pytest.mark.parametrize("dtype,mult", [("fp32", 4), (None, 16)], ids=["f32", "split"])
@pytest.mark.parametrize("tag", ["segn96", "seg3n64x96"])
def test_predict_rows_and_masks_against_the_reference(g, tag, dtype, mult, device):
    y, m = _yolo(g, tag)
    x = torch.rand(*m["shape"], generator=torch.Generator().manual_seed(m["seed"]))
    res = y.predict(x, device=0, dtype=dtype, conf=0.25, iou=0.7)
    assert y.predictor.dtype == (torch.float32 if dtype else X2) and type(y.predictor).__name__ == "SegmentationPredictor"
    _check(g, tag, "", res, y, mult, f"predict {tag} {dtype or 'split'}")
    if dtype is None:
        # a streamed run keeps the device a batch ahead: the masks must not see the next batch's prototypes
        streamed = list(y.predict(x, device=0, conf=0.25, iou=0.7, stream=True, batch=1))
        assert len(streamed) == len(res)
        for a, b in zip(streamed, res):
            assert torch.equal(a.boxes.data, b.boxes.data) and torch.equal(a.masks.data, b.masks.data)
        # half=True: measured, no bar (the 16-bit path runs in the scaled activation domain)
        y2, _ = _yolo(g, tag)
        _check(g, tag, "", y2.predict(x, device=0, half=True, conf=0.25, iou=0.7), y2, mult, f"predict {tag} half", bar=False)


@pytest.mark.parametrize("dtype,mult", [("fp32", 4), (None, 16)], ids=["f32", "split"])
@pytest.mark.parametrize("retina", [False, True], ids=["input", "retina"])
def test_predict_uint8_frame_through_the_letterbox(g, retina, dtype, mult, device):
    y, m = _yolo(g, "segn_u8")
    frame = g["segn_u8__frame"]
    res = y.predict([frame], device=0, dtype=dtype, conf=0.25, iou=0.7, imgsz=m["imgsz"], retina_masks=retina)
    assert tuple(res[0].masks.shape[1:]) == (tuple(frame.shape[:2]) if retina else tuple(m["shape"][2:])) and res[0].orig_shape == tuple(frame.shape[:2])
    _check(g, "segn_u8", "_retina" if retina else "", res, y, mult, f"predict segn_u8 retina={retina} {dtype or 'split'}")


def test_image_without_detections_has_no_masks(g, device):
    y, m = _yolo(g, "seg3n64x96")
    x = torch.rand(*m["shape"], generator=torch.Generator().manual_seed(m["seed"]))
    res = y.predict(x, device=0, conf=0.999)
    assert all(len(r) == 0 and r.masks is None for r in res)


@pytest.mark.parametrize("tag", ["n64", "n128", "sf_n64"])
def test_detection_models_are_unchanged(tag, device):
    e = golden("e2e.npz")
    m = meta(e, tag)
    y = YOLO(m["yaml"].replace("yolov8-", f"yolov8{m['scale']}-"))
    y.model = D.DetectionModel(dict(load_yaml(m["yaml"], m["scale"], m["nc"])), nc=m["nc"], verbose=False)
    y.model.load_state_dict(O.seeded_state_dict(y.model.state_dict(), m["seed"], cls_bias=m["cls_bias"]))
    b, h, w = m["shape"]
    res = y.predict(torch.rand(b, 3, h, w, generator=torch.Generator().manual_seed(m["seed"])), device=0, conf=0.25, iou=0.7)
    assert y.task == "detect" and type(y.predictor).__name__ == "DetectionPredictor"
    counts = [int(k) for k in e[f"{tag}__n"]]
    exp = split_rows(e[f"{tag}__det"], counts)
    for i, r in enumerate(res):
        assert r.masks is None
        rows = r.boxes.data.cpu().numpy()
        assert len(rows) == counts[i] and np.array_equal(rows[:, 5], exp[i][:, 5])
        if len(rows):
            clipped = np.clip(exp[i][:, :4], 0, [w, h, w, h])  # construct_result clips the kept boxes to the image (detect/predict.py:59-73)
            assert box_iou_pairs(rows[:, :4], clipped).min() >= 0.999
