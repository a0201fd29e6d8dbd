"""GPU parity of oriented-box validation against tests/golden/obbval.npz (tools/make_obbval_golden.py: the REAL reference's
``non_max_suppression(rotated=True, multi_label=True)``, ``match_predictions`` on ``batch_probiou`` and ``OBBValidator``).

Bars.  ``dy_val_match_rotated``: ``tp`` EXACTLY the reference's -- the cases are ones the reference decides with a margin (tests/_obbval_util.py:
no same-class pair within M of a threshold, M = 8 x max |iou32 - iou64| over the pairs in [0.4, 0.97], never below the margin of the 300 x 40
case); ``best_label`` the float64 argmax on rows whose float64 best IoU is >= 0.4; ``best_iou`` within M of float64 up to 0.97 and within
M_top above.  ``dy_nms_rotated_ml``: the reference's kept (anchor, class) pairs, order and counts exactly, rows equal in fp32.  End to end:
counts, classes and ``tp`` exact, confidences within the project's row tolerance, the dict the reference's to its 5 digits."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from drone_yolo_amd import YOLO, _lib
from drone_yolo_amd import hip_ops as H
from drone_yolo_amd.engine.validator import OBBValidator
from drone_yolo_amd.nn.tasks import OBBModel
from oracle import drone_yolo_oracle as O
from tests import _obbval_util as V
from tests._util import golden, load_yaml, meta, split_rows
from tests.test_model_gpu import RTOL as _RTOL
from tests.test_obbval_host import MATCH_NAMES, e2e_fixture, match_case, seedless_case, unpack

pytestmark = pytest.mark.gpu
X2 = H.F16X2
RTOL = {**_RTOL, X2: _RTOL[torch.float32]}  # split float16 (22 mantissa bits) is held to fp32's
GUARD = 64  # bytes either side of every output


@pytest.fixture(scope="module")
def g():
    return golden("obbval.npz")


# ---- dy_val_match_rotated ----------------------------------------------------------------------------------------------------------------
def _bufs(c, device, rows=None):
    bufs = H.RNmsBuffers(len(c["counts"]), 1, c["max_det"], device)
    bufs.out.copy_(torch.from_numpy(c["rows"] if rows is None else rows))
    bufs.count.copy_(torch.from_numpy(c["counts"]))
    return bufs


def _labels(c, device):
    return [torch.from_numpy(np.ascontiguousarray(c[k])).to(device) for k in ("tbox", "tcls", "timg")]


def _wrapper(c, device, bufs=None):
    return H.val_match_rotated(bufs or _bufs(c, device), *_labels(c, device), V.IOUV, c["clip"], single_cls=c["single_cls"], want_best=True)


def _guarded(c, device):
    """The entry point itself, writing into views with GUARD poisoned bytes either side: (tp, best_iou, best_label, guards untouched)."""
    B, md, T = len(c["counts"]), c["max_det"], len(V.IOUV)
    bufs = _bufs(c, device)
    tbox, tcls, timg = _labels(c, device)
    padded = torch.zeros((len(tbox), 8), dtype=torch.float32, device=device)
    padded[:, :5] = tbox
    raw = [torch.full((n * size + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=device) for n, size in ((B * md * T, 1), (B * md, 4), (B * md, 4))]
    views = [r[GUARD : len(r) - GUARD] for r in raw]
    thr = (ctypes.c_float * T)(*[float(v) for v in V.IOUV])
    d = _lib.ValMatchRotatedDesc()
    d.rows, d.counts = bufs.out.data_ptr(), bufs.count.data_ptr()
    tcls = tcls.float().contiguous()
    d.tbox, d.tcls, d.timg = padded.data_ptr(), tcls.data_ptr(), timg.data_ptr()
    d.iouv, d.batch, d.max_det, d.n_labels, d.n_iouv = thr, B, md, len(tbox), T
    d.clip_w, d.clip_h, d.single_cls = float(c["clip"][0]), float(c["clip"][1]), int(c["single_cls"])
    d.tp, d.best_iou, d.best_label = (v.data_ptr() for v in views)
    assert _lib.lib().dy_val_match_rotated(ctypes.byref(d), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    clean = all(bool((r[:GUARD] == 0xA5).all()) and bool((r[len(r) - GUARD :] == 0xA5).all()) for r in raw)
    return views[0].view(B, md, T), views[1].view(torch.float32).view(B, md), views[2].view(torch.int32).view(B, md), clean


@pytest.mark.parametrize("name", MATCH_NAMES)
def test_val_match_rotated_against_the_reference(g, name, device):
    c, e = match_case(name)
    B, md = len(c["counts"]), c["max_det"]
    M, M_top = (float(v) for v in g[f"m_{name}__margin"])
    tp_ref = unpack(g, f"m_{name}__tp", (B, md, 10))
    tp, bi, bl = _wrapper(c, device)
    assert H.last_kernel_name() == "val_match_rotated_kernel"
    assert tp.dtype == torch.uint8 and tuple(tp.shape) == (B, md, 10) and bi.dtype == torch.float32 and bl.dtype == torch.int32
    tpn, bin_, bln = tp.cpu().numpy(), bi.cpu().numpy(), bl.cpu().numpy()
    b64, l64 = g[f"m_{name}__best_iou"], g[f"m_{name}__best_label"]
    assert not np.isnan(bin_).any()
    worst, worst_top = 0.0, 0.0
    for i, cnt in enumerate(c["counts"]):
        assert not tpn[i, cnt:].any() and not bin_[i, cnt:].any() and (bln[i, cnt:] == -1).all(), "rows behind the count must be 0 / 0 / -1"
        err = np.abs(bin_[i, :cnt].astype(np.float64) - b64[i, :cnt])
        low = b64[i, :cnt] <= V.BAND_HI
        worst, worst_top = max(worst, float(err[low].max(initial=0.0))), max(worst_top, float(err[~low].max(initial=0.0)))
        sure = b64[i, :cnt] >= V.BAND_LO
        assert np.array_equal(bln[i, :cnt][sure], l64[i, :cnt][sure]), f"{name}: image {i}: best_label is not the float64 argmax"
    print(f"val_match_rotated {name}: max |best_iou - float64| {worst:.3e} (M {M:.3e}), above 0.97 {worst_top:.3e} (M_top {M_top:.3e})")
    assert np.array_equal(tpn.astype(bool), tp_ref), f"{name}: {(tpn.astype(bool) != tp_ref).sum()} tp cells differ from the reference's"
    assert worst <= M and worst_top <= M_top
    # the entry point on guarded views: the same bytes, nothing outside them
    tp2, bi2, bl2, clean = _guarded(c, device)
    assert clean, "bytes outside an output were written"
    assert torch.equal(tp2, tp) and torch.equal(bi2.view(torch.int32), bi.view(torch.int32)) and torch.equal(bl2, bl), "two runs differ"
    tp_only = H.val_match_rotated(_bufs(c, device), *_labels(c, device), V.IOUV, c["clip"], single_cls=c["single_cls"])
    assert torch.equal(tp_only, tp)


@pytest.mark.parametrize("name", MATCH_NAMES)
def test_val_match_rotated_replayed_from_a_captured_graph(name, device):
    c, _ = match_case(name)
    rows2 = c["rows"].copy()
    rows2[:, :, :2] += np.float32(0.37)  # new rows: every centre moved
    labels = _labels(c, device)
    eager = [t.clone() for t in _wrapper(c, device, _bufs(c, device, rows2))]
    bufs = _bufs(c, device)
    first = [t.clone() for t in _wrapper(c, device, bufs)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = H.val_match_rotated(bufs, *labels, V.IOUV, c["clip"], single_cls=c["single_cls"], want_best=True)
    bufs.out.copy_(torch.from_numpy(rows2))
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(outs, eager)), "the replay did not give the new rows' result"
    if c["counts"].max() > 1 and name != "degenerate":
        assert not torch.equal(first[1], eager[1]), "the new rows must score differently"


@pytest.mark.parametrize("name", ["full_stage", "bound"])
def test_val_match_rotated_full_stage_and_layout_bound(name, device):
    """A stage filled exactly to capacity (257 labels at a step of 256) and the largest dynamic LDS request (max_det 4096: 36 bytes per
    detection), against the float64 rule; the outputs start poisoned, so every element is written."""
    c, tp64, best64 = seedless_case(name)
    tp, bi, bl, clean = _guarded(c, device)
    assert H.last_kernel_name() == "val_match_rotated_kernel" and clean
    tpn, bin_, bln = tp.cpu().numpy()[0], bi.cpu().numpy()[0], bl.cpu().numpy()[0]
    assert np.array_equal(bln, best64), "best_label is not the float64 argmax"
    assert np.array_equal(tpn, tp64.astype(np.uint8))
    hit = tp64.any(1)
    dup = np.zeros_like(hit) if name == "bound" else np.arange(4) == 3  # (the second copy scores as the first and loses the label)
    assert (bin_[hit | dup] > 0.99).all() and not bin_[~(hit | dup)].any()


def test_no_labels_and_argument_checks(device):
    c, _ = match_case("few")
    bufs = _bufs(c, device)
    empty = torch.zeros((0, 5), device=device)
    tp, bi, bl = H.val_match_rotated(bufs, empty, torch.zeros(0, device=device), torch.zeros(0, device=device), V.IOUV, c["clip"], want_best=True)
    assert not tp.any() and not bi.any() and bool((bl == -1).all())
    with pytest.raises(ValueError, match="xywhr"):
        H.val_match_rotated(bufs, torch.zeros((3, 4), device=device), torch.zeros(3, device=device), torch.zeros(3, device=device), V.IOUV, c["clip"])
    with pytest.raises(ValueError, match="7-column"):
        H.val_match_rotated(H.NmsBuffers(3, 1, 8, device), *_labels(c, device), V.IOUV, c["clip"])


# ---- dy_nms_rotated_ml -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _nms_case(name):
    g = golden("obbval.npz")
    pred, theta = V.nms_inputs(name, int(g[f"n_{name}__seed"]))
    return pred, theta, dict(V.NMS_CASES[name][4]), V.NMS_CASES[name][2]


def _run_nms(pred, theta, kw, nc, bufs=None):
    return H.nms_rotated_ml(pred, theta, V.CONF, V.IOU, nc=nc, bufs=bufs, **{"max_det": 300, **kw})


@pytest.mark.parametrize("name", list(V.NMS_CASES))
def test_nms_rotated_ml_against_the_reference(g, name, device):
    pred, theta, kw, nc = _nms_case(name)
    pd, td = pred.to(device), theta.to(device)
    bufs = _run_nms(pd, td, kw, nc)
    assert H.last_kernel_name() == ("nms_rotated_kernel" if nc == 1 else "nms_rotated_ml_kernel")
    counts = [int(k) for k in g[f"n_{name}__n"]]
    max_det = kw.get("max_det", 300)
    assert tuple(bufs.out.shape) == (len(counts), max_det, 7) and bufs.cpa == nc
    assert bufs.count.tolist() == counts, f"{name}: kept {bufs.count.tolist()}, the reference {counts}"
    exp_idx, exp_rows = split_rows(g[f"n_{name}__idx"], counts), split_rows(g[f"n_{name}__rows"], counts)
    out, index = bufs.out.cpu().numpy(), bufs.index.cpu().numpy()
    for b, k in enumerate(counts):
        assert np.array_equal(index[b, :k], exp_idx[b]), f"{name}: image {b}: out_index must hold the reference's anchors in its order"
        assert (index[b, k:] == -1).all() and (out[b, k:] == 0).all(), "rows behind the count must be zero, their index -1"
        # the reference's row is (x, y, w, h, conf, cls, theta); ours (x, y, w, h, theta, conf, cls): all copies, equal in fp32
        assert np.array_equal(out[b, :k, :4], exp_rows[b][:, :4]) and np.array_equal(out[b, :k, 5:7], exp_rows[b][:, 4:6])
        assert np.array_equal(out[b, :k, 4], exp_rows[b][:, 6])
    again = _run_nms(pd, td, kw, nc)
    assert again is not bufs and torch.equal(again.out.view(torch.int32), bufs.out.view(torch.int32)) and torch.equal(again.index, bufs.index) and torch.equal(again.count, bufs.count)
    reused = _run_nms(pd, td, kw, nc, bufs=again)
    assert reused is again and torch.equal(reused.out.view(torch.int32), bufs.out.view(torch.int32))
    if name == "two":
        assert index[0, :2].tolist() == [17, 17] and out[0, :2, 6].tolist() == [0.0, 2.0]
    if name == "nc1":  # identical to the single-label entry point
        single = H.nms_rotated(pd, td, V.CONF, V.IOU, nc=1)
        assert torch.equal(single.out.view(torch.int32), bufs.out.view(torch.int32)) and torch.equal(single.index, bufs.index) and torch.equal(single.count, bufs.count)
    if name == "lds_cap":
        assert pred.shape[2] < _lib.lib().dy_nms_rotated_lds_cap() < V.pair_counts(pred, nc)[0]


def test_nms_rotated_ml_ignores_the_descriptors_multi_label_field_and_takes_a_class_mask(g, device):
    pred, theta, kw, nc = _nms_case("chunks")
    pd, td = pred.to(device), theta.to(device)
    ref = _run_nms(pd, td, kw, nc)
    bufs = H.RNmsBuffers(pd.shape[0], pd.shape[2], 300, device, candidates_per_anchor=nc)
    d = H._nms_desc(pd, bufs, nc, V.CONF, V.IOU, 30000, 7680.0, False, None, False, False)  # multi_label = 0 in the descriptor
    assert _lib.lib().dy_nms_rotated_ml(ctypes.byref(d), td.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    assert torch.equal(bufs.out.view(torch.int32), ref.out.view(torch.int32)) and torch.equal(bufs.count, ref.count)
    assert H.RNmsBuffers(2, 100, 300, device).workspace.numel() == _lib.lib().dy_nms_rotated_workspace_bytes(2, 100), "the default sizes are today's"
    mask = torch.tensor([1, 0, 1], dtype=torch.uint8, device=device)
    only = H.nms_rotated_ml(pd, td, V.CONF, V.IOU, nc=nc, classes_mask=mask)
    k = only.count.tolist()
    assert sum(k) > 0 and all(int(c) in (0, 2) for b in range(len(k)) for c in only.out[b, : k[b], 6].tolist())


# ---- end to end --------------------------------------------------------------------------------------------------------------------------
def _yolo_and_data(g, tag):
    m = meta(g, tag)
    y = YOLO(m["yaml"].replace("yolov8-", f"yolov8{m['scale']}-"))
    y.model = OBBModel(dict(load_yaml(m["yaml"], m["scale"], m["nc"])), nc=m["nc"], verbose=False)
    y.model.load_state_dict(O.seeded_state_dict(y.model.state_dict(), m["seed"], cls_bias=m["cls_bias"]))
    assert y.task == "obb"
    data = dict(img=V.e2e_images(m["seed"], m["shape"][0]), batch_idx=torch.from_numpy(g[f"{tag}__batch_idx"]), cls=torch.from_numpy(g[f"{tag}__cls"]).view(-1, 1),
                bboxes=torch.from_numpy(g[f"{tag}__bboxes"]))
    return y, m, data


def _val(y, data, m, kept, **kw):
    def make(args):
        v = OBBValidator(args)
        kept.append(v)
        return v

    return y.val(validator=make, data=data, batch=m["batch"], conf=m["conf"], iou=m["iou"], device=0, **kw)


@pytest.mark.parametrize("dtype", ["fp32", None], ids=["f32", "split"])
@pytest.mark.parametrize("tag", list(V.E2E))
def test_val_end_to_end_against_the_reference(g, tag, dtype, device):
    y, m, data = _yolo_and_data(g, tag)
    _, counts_ref, rows_ref, tp_ref, res_ref = e2e_fixture(g, tag)
    n = m["shape"][0]
    kept = []
    kw = dict(dtype=dtype) if dtype else {}
    dev = _val(y, data, m, kept, device_match=True, **kw)
    assert y.metrics is dev and list(dev) == list(OBBValidator().metrics.keys) + ["fitness"] and not any(k.startswith("val/") for k in dev)
    assert y.predictor is None
    host = _val(y, data, m, kept, device_match=False, **kw)
    ref = {k: round(float(v), 5) for k, v in res_ref.items()}
    print(tag, dtype or "split", "device", dev, "host", host, "reference", ref)
    vd, vh = kept
    assert vd.device_match and not vh.device_match
    counts = [int(k) for k in vd.last_counts]
    print(tag, dtype or "split", "kept", counts, "the reference", counts_ref.tolist())
    assert counts == counts_ref.tolist() and [int(k) for k in vh.last_counts] == counts
    st = {k: np.concatenate(v, 0) for k, v in vd.last_stats.items()}
    sh = {k: np.concatenate(v, 0) for k, v in vh.last_stats.items()}
    for k in st:
        assert st[k].dtype == sh[k].dtype and np.array_equal(st[k], sh[k]), f"last_stats[{k}] differs between device_match=True and False"
    tol = RTOL[torch.float32 if dtype else X2]
    o, worst = 0, 0.0
    for i in range(n):
        k = counts[i]
        assert np.array_equal(st["pred_cls"][o : o + k], rows_ref[i, :k, 6]), f"image {i}: classes differ from the reference's"
        worst = max(worst, float(np.abs(st["conf"][o : o + k] - rows_ref[i, :k, 5]).max()))
        assert np.array_equal(st["tp"][o : o + k], tp_ref[i, :k]), f"image {i}: tp differs from the reference's"
        o += k
    print(tag, dtype or "split", f"max |conf - reference| {worst:.3e} (bar {tol:.1e})")
    assert worst <= tol
    assert np.array_equal(st["target_cls"], g[f"{tag}__cls"])
    assert dev == host, "device_match=True and False disagree"
    assert dev == ref, {k: (dev[k], ref[k]) for k in ref if dev[k] != ref[k]}
    plain = y.val(data=data, batch=m["batch"], conf=m["conf"], iou=m["iou"], device=0, **kw)  # without validator=: the task's own
    assert plain == dev and y.metrics is plain


def test_val_half_runs_and_fp8_is_refused(g, device):
    y, m, data = _yolo_and_data(g, "ovp2")
    out = _val(y, data, m, [], half=True)
    print("ovp2 half=True", out)
    assert y.metrics is out and all(np.isfinite(v) for v in out.values()) and len(out) == 5
    with pytest.raises(NotImplementedError, match="OBB is built for"):
        y.val(data=data, dtype="fp8", device=0)
