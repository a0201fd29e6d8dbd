"""GPU parity of pose validation against tests/golden/poseval.npz (tools/make_poseval_golden.py: the REAL reference's ``kpt_iou``,
``match_predictions`` and ``PoseValidator``).

Bars.  ``dy_val_oks_match``: ``tp`` EXACTLY the reference's -- the cases are ones the reference decides with a margin (tests/_poseval_util.py:
no same-class pair within M of a threshold, M = 8 x max |oks32 - oks64| over the pairs at or above 0.4, never below the margin of the 300 x 40
case); ``best_label`` the float64 argmax on rows whose float64 best OKS is >= 0.4; ``best_iou`` within M of float64.  End to end: counts,
classes, ``tp`` and ``tp_p`` exact, confidences within 1e-4 of the scale (1), the dict the reference's to its 5 digits."""
import ctypes

import numpy as np
import pytest
import torch

from drone_yolo_amd import YOLO, _lib
from drone_yolo_amd import hip_ops as H
from drone_yolo_amd.engine.validator import PoseValidator
from drone_yolo_amd.nn.tasks import PoseModel
from oracle import drone_yolo_oracle as O
from tests import _poseval_util as V
from tests._util import golden, load_yaml, meta
from tests.test_poseval_host import MATCH_NAMES, e2e_fixture, match_case, seedless_case, unpack

pytestmark = pytest.mark.gpu
GUARD = 64  # bytes either side of every output
CONF_TOL = 1e-4  # of the scale: a confidence is at most 1


@pytest.fixture(scope="module")
def g():
    return golden("poseval.npz")


# ---- dy_val_oks_match --------------------------------------------------------------------------------------------------------------------
def _bufs(c, device, anchors=1, index=None):
    bufs = H.NmsBuffers(len(c["counts"]), anchors, c["max_det"], device)
    bufs.out.copy_(torch.from_numpy(c["rows"]))
    bufs.count.copy_(torch.from_numpy(c["counts"]))
    bufs.index.fill_(-1) if index is None else bufs.index.copy_(torch.from_numpy(index))
    return bufs


def _labels(c, device):
    return [torch.from_numpy(np.ascontiguousarray(c[k])).to(device) for k in ("tbox", "tkpt", "tcls", "timg")]


def _gathered(c, device, kpts=None):
    B, md = len(c["counts"]), c["max_det"]
    return torch.from_numpy(np.ascontiguousarray(c["kpts"] if kpts is None else kpts)).reshape(B, md, -1).to(device)


def _wrapper(c, device, bufs=None, kpts=None):
    """The gathered-rows form through hip_ops."""
    return H.val_oks_match(bufs or _bufs(c, device), _gathered(c, device) if kpts is None else kpts, c["kpt_shape"], *_labels(c, device),
                           V.sigma_of(c["kpt_shape"]), V.IOUV, c["clip"], single_cls=c["single_cls"], want_best=True)


def _dense(c, device):
    """The dense-plus-index form through hip_ops: the (B, C, A) tensor and an index whose entries beyond the counts are poison."""
    pred, index = V.dense_form(c)
    bufs = _bufs(c, device, anchors=pred.shape[2], index=index)
    return H.val_oks_match(bufs, torch.from_numpy(pred).to(device), c["kpt_shape"], *_labels(c, device), V.sigma_of(c["kpt_shape"]), V.IOUV, c["clip"],
                           nc=V.NC, single_cls=c["single_cls"], want_best=True)


def _desc(c, device, keep):
    """The entry point's descriptor in the gathered form, outputs in views with GUARD poisoned bytes either side."""
    B, md, T = len(c["counts"]), c["max_det"], len(V.IOUV)
    nkpt, ndim = c["kpt_shape"]
    bufs, kpts = _bufs(c, device), _gathered(c, device)
    tbox, tkpt, tcls, timg = _labels(c, device)
    tcls = tcls.float().contiguous()
    raw = [torch.full((n * size + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=device) for n, size in ((B * md * T, 1), (B * md, 4), (B * md, 4))]
    views = [r[GUARD : len(r) - GUARD] for r in raw]
    thr = (ctypes.c_float * T)(*[float(v) for v in V.IOUV])
    sg = (ctypes.c_float * nkpt)(*[float(v) for v in V.sigma_of(c["kpt_shape"])])
    d = _lib.ValOksMatchDesc()
    d.rows, d.counts, d.kpts, d.index = bufs.out.data_ptr(), bufs.count.data_ptr(), kpts.data_ptr(), None
    d.stride_b, d.stride_ch, d.stride_d, d.anchors = md * nkpt * ndim, 1, nkpt * ndim, 0
    d.tbox, d.tkpt, d.tcls, d.timg = tbox.data_ptr(), tkpt.data_ptr(), tcls.data_ptr(), timg.data_ptr()
    d.sigma, d.iouv = sg, thr
    d.batch, d.max_det, d.n_labels, d.n_iouv, d.nkpt, d.ndim = B, md, len(tbox), T, nkpt, ndim
    d.clip_w, d.clip_h, d.single_cls = float(c["clip"][0]), float(c["clip"][1]), int(c["single_cls"])
    d.tp, d.best_iou, d.best_label = (v.data_ptr() for v in views)
    keep.extend((bufs, kpts, tbox, tkpt, tcls, timg, thr, sg, raw))
    return d, raw, views


def _call(d):
    rc = _lib.lib().dy_val_oks_match(ctypes.byref(d), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


def _guarded(c, device):
    """The entry point itself: (tp, best_iou, best_label, guards untouched)."""
    B, md, T = len(c["counts"]), c["max_det"], len(V.IOUV)
    keep = []
    d, raw, views = _desc(c, device, keep)
    assert _call(d) == 0
    clean = all(bool((r[:GUARD] == 0xA5).all()) and bool((r[len(r) - GUARD :] == 0xA5).all()) for r in raw)
    return views[0].view(B, md, T), views[1].view(torch.float32).view(B, md), views[2].view(torch.int32).view(B, md), clean


@pytest.mark.parametrize("name", MATCH_NAMES)
def test_val_oks_match_against_the_reference(g, name, device):
    c, e = match_case(name)
    B, md = len(c["counts"]), c["max_det"]
    M = float(g[f"m_{name}__margin"][0])
    tp_ref = unpack(g, f"m_{name}__tp", (B, md, 10))
    tp, bi, bl = _wrapper(c, device)
    assert H.last_kernel_name() == "val_oks_kernel"
    assert tp.dtype == torch.uint8 and tuple(tp.shape) == (B, md, 10) and bi.dtype == torch.float32 and bl.dtype == torch.int32
    tpn, bin_, bln = tp.cpu().numpy(), bi.cpu().numpy(), bl.cpu().numpy()
    b64, l64 = g[f"m_{name}__best_iou"], g[f"m_{name}__best_label"]
    assert not np.isnan(bin_).any()
    worst = 0.0
    for i, cnt in enumerate(c["counts"]):
        assert not tpn[i, cnt:].any() and not bin_[i, cnt:].any() and (bln[i, cnt:] == -1).all(), "rows behind the count must be 0 / 0 / -1"
        worst = max(worst, float(np.abs(bin_[i, :cnt].astype(np.float64) - b64[i, :cnt]).max(initial=0.0)))
        sure = b64[i, :cnt] >= V.BAND_LO
        assert np.array_equal(bln[i, :cnt][sure], l64[i, :cnt][sure]), f"{name}: image {i}: best_label is not the float64 argmax"
    print(f"val_oks_match {name}: max |best_iou - float64| {worst:.3e} (M {M:.3e})")
    assert np.array_equal(tpn.astype(bool), tp_ref), f"{name}: {(tpn.astype(bool) != tp_ref).sum()} tp cells differ from the reference's"
    assert worst <= M
    # the entry point on guarded views: the same bytes, nothing outside them
    tp2, bi2, bl2, clean = _guarded(c, device)
    assert clean, "bytes outside an output were written"
    assert torch.equal(tp2, tp) and torch.equal(bi2.view(torch.int32), bi.view(torch.int32)) and torch.equal(bl2, bl), "two runs differ"
    # the dense-plus-index addressing: the same bits
    tp3, bi3, bl3 = _dense(c, device)
    assert torch.equal(tp3, tp) and torch.equal(bi3.view(torch.int32), bi.view(torch.int32)) and torch.equal(bl3, bl), "the dense and the gathered addressings differ"
    tp_only = H.val_oks_match(_bufs(c, device), _gathered(c, device), c["kpt_shape"], *_labels(c, device), V.sigma_of(c["kpt_shape"]), V.IOUV, c["clip"],
                              single_cls=c["single_cls"])
    assert torch.equal(tp_only, tp)


@pytest.mark.parametrize("name", ["val300", "few", "invisible", "kpt4x2"])
def test_val_oks_match_replayed_from_a_captured_graph(name, device):
    c, _ = match_case(name)
    kpts2 = c["kpts"].copy()
    kpts2[..., :2] += np.float32(0.9)  # new rows: every keypoint moved
    eager = [t.clone() for t in _wrapper(c, device, kpts=_gathered(c, device, kpts2))]
    bufs, kpts = _bufs(c, device), _gathered(c, device)
    labels = _labels(c, device)
    first = [t.clone() for t in _wrapper(c, device, bufs, kpts)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = H.val_oks_match(bufs, kpts, c["kpt_shape"], *labels, V.sigma_of(c["kpt_shape"]), V.IOUV, c["clip"], single_cls=c["single_cls"], want_best=True)
    kpts.copy_(_gathered(c, device, kpts2))
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(outs, eager)), "the replay did not give the new rows' result"
    assert not torch.equal(first[1], eager[1]), "the new rows must score differently"


@pytest.mark.parametrize("name", ["full_stage", "bound"])
def test_val_oks_match_full_stage_and_layout_bound(name, device):
    """A stage filled exactly to capacity (65 labels at a step of 64) and the largest dynamic LDS request (max_det 4096 at 32 keypoints), against
    the float64 rule; the outputs start poisoned, so every element is written."""
    c, tp64, best64 = seedless_case(name)
    tp, bi, bl, clean = _guarded(c, device)
    assert H.last_kernel_name() == "val_oks_kernel" and clean
    tpn, bin_, bln = tp.cpu().numpy()[0], bi.cpu().numpy()[0], bl.cpu().numpy()[0]
    assert np.array_equal(bln, best64), "best_label is not the float64 argmax"
    assert np.array_equal(tpn, tp64.astype(np.uint8))
    hit = tp64.any(1)
    dup = np.zeros_like(hit) if name == "bound" else np.arange(4) == 3  # (the second copy scores as the first and loses the label)
    assert (bin_[hit | dup] > 0.999).all() and (bin_[~(hit | dup)] < 1e-6).all()


def test_no_labels_and_wrapper_argument_checks(device):
    c, _ = match_case("few")
    bufs, kpts = _bufs(c, device), _gathered(c, device)
    sg = V.sigma_of(c["kpt_shape"])
    none = [torch.zeros((0, 4), device=device), torch.zeros((0, 17, 3), device=device), torch.zeros(0, device=device), torch.zeros(0, device=device)]
    tp, bi, bl = H.val_oks_match(bufs, kpts, c["kpt_shape"], *none, sg, V.IOUV, c["clip"], want_best=True)
    assert not tp.any() and not bi.any() and bool((bl == -1).all())
    labels = _labels(c, device)
    with pytest.raises(ValueError, match="tkpt"):
        H.val_oks_match(bufs, kpts, c["kpt_shape"], labels[0], labels[1][:, :5], *labels[2:], sg, V.IOUV, c["clip"])
    with pytest.raises(ValueError, match="gathered form"):
        H.val_oks_match(bufs, kpts[:, :, :-1].contiguous(), c["kpt_shape"], *labels, sg, V.IOUV, c["clip"])
    with pytest.raises(ValueError, match="dense form"):
        H.val_oks_match(bufs, kpts, c["kpt_shape"], *labels, sg, V.IOUV, c["clip"], nc=3)
    with pytest.raises(NotImplementedError, match="at most 32"):
        H.val_oks_match(bufs, kpts, (33, 2), *labels, [0.1] * 33, V.IOUV, c["clip"])
    with pytest.raises(ValueError, match="kpt_shape"):
        H.val_oks_match(bufs, kpts, (17, 4), *labels, sg, V.IOUV, c["clip"])


def test_every_refusal_returns_without_a_launch_and_leaves_the_outputs_untouched(device):
    c, _ = match_case("few")
    keep = []
    d, raw, _ = _desc(c, device, keep)
    tbox_ptr, kpts_ptr = d.tbox, d.kpts
    big_sigma = (ctypes.c_float * 64)(*([0.05] * 64))
    cases = [("kpts", None, -1), ("max_det", 0, -1), ("max_det", 4097, -1), ("n_iouv", 17, -1), ("ndim", 4, -1), ("nkpt", _lib.OKS_MAX_KPT + 1, -2),
             ("tbox", tbox_ptr + 4, -1)]
    for field, value, code in cases:
        old = getattr(d, field)
        if field == "nkpt":
            d.sigma = big_sigma
        setattr(d, field, value)
        assert _call(d) == code, f"{field} = {value}"
        assert field.encode() in _lib.lib().dy_last_error_string() or field == "kpts"
        setattr(d, field, old)
        assert all(bool((r == 0xA5).all()) for r in raw), f"{field} = {value}: an output was written"
    assert d.kpts == kpts_ptr and _call(d) == 0 and not all(bool((r == 0xA5).all()) for r in raw), "the restored descriptor runs"


# ---- end to end --------------------------------------------------------------------------------------------------------------------------
def _yolo_and_data(g, tag):
    m = meta(g, tag)
    y = YOLO(m["yaml"].replace("yolov8-", f"yolov8{m['scale']}-"))
    y.model = PoseModel(dict(load_yaml(m["yaml"], m["scale"], m["nc"])), nc=m["nc"], verbose=False)
    y.model.load_state_dict(O.seeded_state_dict(y.model.state_dict(), m["seed"], cls_bias=m["cls_bias"]))
    assert y.task == "pose"
    data = dict(img=V.e2e_images(m["seed"], m["shape"][0]), batch_idx=torch.from_numpy(g[f"{tag}__batch_idx"]), cls=torch.from_numpy(g[f"{tag}__cls"]).view(-1, 1),
                bboxes=torch.from_numpy(g[f"{tag}__bboxes"]), keypoints=torch.from_numpy(g[f"{tag}__keypoints"]))
    return y, m, data


def _val(y, data, m, kept, **kw):
    def make(args):
        v = PoseValidator(args)
        kept.append(v)
        return v

    return y.val(validator=make, data=data, batch=m["batch"], conf=m["conf"], iou=m["iou"], device=0, **kw)


@pytest.mark.parametrize("dtype", ["fp32", None], ids=["f32", "split"])
@pytest.mark.parametrize("tag", list(V.E2E))
def test_val_end_to_end_against_the_reference(g, tag, dtype, device):
    y, m, data = _yolo_and_data(g, tag)
    _, counts_ref, rows_ref, _, tp_ref, tpp_ref, res_ref = e2e_fixture(g, tag)
    n = m["shape"][0]
    kept = []
    kw = dict(dtype=dtype) if dtype else {}
    dev = _val(y, data, m, kept, device_match=True, **kw)
    assert y.metrics is dev and list(dev) == list(PoseValidator().metrics.keys) + ["fitness"] and not any(k.startswith("val/") for k in dev)
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
    assert list(st) == ["tp", "tp_p", "conf", "pred_cls", "target_cls"]
    for k in st:
        assert st[k].dtype == sh[k].dtype and np.array_equal(st[k], sh[k]), f"last_stats[{k}] differs between device_match=True and False"
    o, worst = 0, 0.0
    for i in range(n):
        k = counts[i]
        assert np.array_equal(st["pred_cls"][o : o + k], rows_ref[i, :k, 5]), f"image {i}: classes differ from the reference's"
        worst = max(worst, float(np.abs(st["conf"][o : o + k] - rows_ref[i, :k, 4]).max()))
        assert np.array_equal(st["tp"][o : o + k], tp_ref[i, :k]), f"image {i}: tp differs from the reference's"
        assert np.array_equal(st["tp_p"][o : o + k], tpp_ref[i, :k]), f"image {i}: tp_p differs from the reference's"
        o += k
    print(tag, dtype or "split", f"max |conf - reference| {worst:.3e} (bar {CONF_TOL:.1e})")
    assert worst <= CONF_TOL
    assert np.array_equal(st["target_cls"], g[f"{tag}__cls"])
    assert dev == host, "device_match=True and False disagree"
    assert dev == ref, {k: (dev[k], ref[k]) for k in ref if dev[k] != ref[k]}
    plain = y.val(data=data, batch=m["batch"], conf=m["conf"], iou=m["iou"], device=0, **kw)  # without validator=: the task's own
    assert plain == dev and y.metrics is plain


def test_val_half_runs_and_fp8_is_refused(g, device):
    y, m, data = _yolo_and_data(g, "pvp2")
    out = _val(y, data, m, [], half=True)
    print("pvp2 half=True", out)
    assert y.metrics is out and all(np.isfinite(v) for v in out.values()) and len(out) == 9
    with pytest.raises(NotImplementedError, match="Pose is built for"):
        y.val(data=data, dtype="fp8", device=0)
