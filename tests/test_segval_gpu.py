"""GPU: ``dy_val_mask_match`` against the float64 evaluation of tests/_segval_util.py at run time and against the REAL reference's recorded
results (tests/golden/segval.npz), and ``YOLO.val`` of the segmentation models end to end.  Nothing is compared with the code under test.

Kernel bars: the integer counts (inter, area_pred, area_gt) equal the float64 counts exactly — every case is drawn (next seed otherwise)
so that no in-crop pixel is *unsure* (|v| below the worst-case fp32 rounding of the dot product) and no crop edge lies within 1e-2 of an
integer; ``best_iou`` is bit-equal to the fp32 expression on those counts, ``best_label`` equal, ``tp_m`` equal to the restated rule and,
where no detection has two same-class labels tied at an IoU >= 0.5, to ``match_predictions``; rows >= count are 0 / 0 / -1; the guard bytes
around every output stay 0xA5.

End to end (``sv_*``), fp32 and split float16.  ``device_match=True`` and ``False`` return the same dict.  Per image whose kept rows are
the reference's (same classes, confidences within 1e-4), ``tp`` and ``tp_m`` equal the recorded matrices.  The dict against the
reference's ``results_dict``: 1e-4 on every entry, (B) and (M) alike — the bar tests/test_train_gpu.py::
test_validator_scores_a_model_against_its_own_detections puts on the box fitness; the dict itself is rounded to 5 digits.
Measured on one MI355X: see DESIGN §18.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import drone_yolo_amd._lib as L
from drone_yolo_amd import YOLO
from drone_yolo_amd import hip_ops as H
from drone_yolo_amd.engine.validator import SegmentationValidator
from drone_yolo_amd.nn.tasks import SegmentationModel
from drone_yolo_amd.utils.metrics import match_predictions
from oracle import drone_yolo_oracle as O
from tests._segval_util import IOUV, case_expected, case_inputs, edges_ok
from tests._util import golden, load_yaml, meta

pytestmark = pytest.mark.gpu
GUARD = 256

# name -> keyword arguments of case_inputs (without the seed): the smallest shapes at which each path can go wrong
CASES = {
    "one_image": dict(grid=(8, 8), ratio=1, in_hw=(32, 32), max_det=4, counts=[3], n_labels=[2]),
    "rows_or_labels_missing": dict(grid=(16, 24), ratio=2, in_hw=(64, 96), max_det=4, counts=[4, 0, 0], n_labels=[0, 3, 0]),
    "all_rows_kept": dict(grid=(16, 24), ratio=2, in_hw=(64, 96), max_det=8, counts=[8], n_labels=[3]),
    "max_det_300": dict(grid=(12, 20), ratio=1, in_hw=(48, 80), max_det=300, counts=[300], n_labels=[6]),
    "labels_255_u8": dict(grid=(20, 20), ratio=1, in_hw=(80, 80), max_det=8, counts=[6], n_labels=[255], one_pixel_labels=True),
    "labels_300_i32": dict(grid=(20, 20), ratio=1, in_hw=(80, 80), max_det=8, counts=[6], n_labels=[300], one_pixel_labels=True, map_dtype=np.int32),
    "labels_300_i32_ratio2": dict(grid=(40, 40), ratio=2, in_hw=(80, 80), max_det=8, counts=[5], n_labels=[300], one_pixel_labels=True, map_dtype=np.int32),
    "empty_label_and_pred": dict(grid=(8, 8), ratio=1, in_hw=(32, 32), max_det=4, counts=[3], n_labels=[3], empty_label=True, empty_pred=True),
    "degenerate_boxes": dict(grid=(10, 13), ratio=1, in_hw=(40, 52), max_det=8, counts=[3, 8], n_labels=[2, 3], degenerate=(1, 6)),
    "single_cls": dict(grid=(16, 24), ratio=2, in_hw=(64, 96), max_det=8, counts=[5, 6], n_labels=[3, 3], single_cls=True),
    "label_slices_differ": dict(grid=(16, 24), ratio=1, in_hw=(64, 96), max_det=8, counts=[5, 6], n_labels=[2, 5]),
}


NEED_TP = {"one_image", "all_rows_kept", "max_det_300", "single_cls", "label_slices_differ"}  # cases that must hold a true tp_m entry


def _drawn(kw, base=4000, need_tp=False):
    """The first seed from ``base`` on whose case has no unsure in-crop pixel and clear crop edges (so the float64 counts are THE counts);
    ``need_tp``: and at least one true ``tp_m`` entry in the float64 evaluation (the case can tell a match from none)."""
    for seed in range(base, base + 400):
        c = case_inputs(seed, **kw)
        e = case_expected(c)
        if e["unsure"] == 0 and edges_ok(c) and (e["tp_m"].any() or not need_tp):
            return c, e
    raise RuntimeError("no seed met the conditions")


_CACHE = {}


def _case(name):
    if name not in _CACHE:  # computed once, shared, left unchanged
        _CACHE[name] = _drawn(CASES[name], need_tp=name in NEED_TP)
    return _CACHE[name]


def _launch(c, device, l_cap=None, iouv=IOUV):
    """dy_val_mask_match on a case through the C entry, every output carved out of one 0xA5-filled buffer with guard gaps."""
    B, md = len(c["counts"]), c["max_det"]
    mh, mw = c["grid"]
    l_cap = l_cap or max(max(c["n_labels"]), 1)
    nt = len(iouv)
    protos = c["protos"].to(device).contiguous()
    side = torch.cat([torch.from_numpy(c["boxes"]), c["coef"]], 2).to(device).contiguous()
    rows = torch.from_numpy(c["rows"]).to(device)
    counts = torch.from_numpy(c["counts"]).to(device)
    maps = torch.from_numpy(c["maps"]).to(device)
    tcls = torch.from_numpy(c["tcls"]).to(device)
    loff = H.label_offsets(torch.from_numpy(c["timg"]).to(device), B)
    sizes = dict(tp_m=B * md * nt, best_iou=B * md * 4, best_label=B * md * 4, area_gt=B * l_cap * 4, inter=B * md * l_cap * 4, area_pred=B * md * 4)
    offs, o = {}, GUARD
    for k, n in sizes.items():
        offs[k] = o
        o = (o + n + GUARD + 15) // 16 * 16
    buf = torch.full((o + GUARD,), 0xA5, dtype=torch.uint8, device=device)
    d = L.ValMaskMatchDesc()
    d.protos, d.side, d.rows, d.counts, d.map, d.loff = protos.data_ptr(), side.data_ptr(), rows.data_ptr(), counts.data_ptr(), maps.data_ptr(), loff.data_ptr()
    d.tcls = tcls.data_ptr() if tcls.numel() else None
    thr = (C.c_float * nt)(*[float(v) for v in iouv])
    d.iouv = thr
    d.batch, d.max_det, d.nm, d.mh, d.mw, d.ld_p, d.gh, d.gw = B, md, 32, mh, mw, 32, maps.shape[1], maps.shape[2]
    d.map_dtype = L.DY_MAP_U8 if maps.dtype == torch.uint8 else L.DY_MAP_I32
    d.n_labels, d.l_cap, d.n_iouv, d.in_w, d.in_h, d.single_cls = int(tcls.numel()), l_cap, nt, c["in_hw"][1], c["in_hw"][0], int(c["single_cls"])
    for k in sizes:
        setattr(d, k, buf.data_ptr() + offs[k])
    rc = L.lib().dy_val_mask_match(C.byref(d), None)
    torch.cuda.synchronize()
    assert rc == 0, L.lib().dy_last_error_string()
    host = buf.cpu().numpy()
    used = np.zeros(len(host), bool)
    out = {}
    for k, n in sizes.items():
        used[offs[k] : offs[k] + n] = True
        raw = host[offs[k] : offs[k] + n]
        out[k] = raw.view(np.float32 if k == "best_iou" else np.uint8 if k == "tp_m" else np.int32)
    assert (host[~used] == 0xA5).all(), "guard bytes were overwritten"
    out["tp_m"] = out["tp_m"].reshape(B, md, nt)
    out["inter"] = out["inter"].reshape(B, md, l_cap)
    out["area_gt"] = out["area_gt"].reshape(B, l_cap)
    for k in ("best_iou", "best_label", "area_pred"):
        out[k] = out[k].reshape(B, md)
    return out


def _check(c, e, got):
    assert np.array_equal(got["inter"], e["inter"]), "inter differs from the float64 counts"
    assert np.array_equal(got["area_pred"], e["area_pred"]) and np.array_equal(got["area_gt"], e["area_gt"])
    assert np.array_equal(got["best_iou"].view(np.uint32), e["best_iou"].view(np.uint32)), "best_iou is not bit-equal to the fp32 expression on the counts"
    assert np.array_equal(got["best_label"], e["best_label"])
    assert set(np.unique(got["tp_m"])) <= {0, 1} and np.array_equal(got["tp_m"].astype(bool), e["tp_m"])
    off = 0
    for b, k in enumerate(c["counts"]):
        nl = c["n_labels"][b]
        assert not got["tp_m"][b, k:].any() and not got["best_iou"][b, k:].any() and (got["best_label"][b, k:] == -1).all()
        assert not got["inter"][b, k:].any() and not got["area_pred"][b, k:].any() and not got["area_gt"][b, nl:].any()
        if k and nl and not e["tie"]:
            pc = np.zeros(k, np.float32) if c["single_cls"] else c["rows"][b, :k, 5]
            tc = c["tcls"][off : off + nl]
            assert np.array_equal(got["tp_m"][b, :k].astype(bool), match_predictions(pc, tc, e["iou"][b], IOUV))
        off += nl


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_cases_against_the_float64_evaluation(name, device):
    c, e = _case(name)
    got = _launch(c, device)
    print(name, {"tp_m": int(got["tp_m"].sum()), "best_iou_max": float(got["best_iou"].max()), "area_pred": got["area_pred"].ravel()[:8].tolist(), "tie": e["tie"]})
    _check(c, e, got)
    if name == "empty_label_and_pred":  # IoU exactly 0 in both cases, no threshold passes
        assert got["area_pred"][0, 0] == 0 and got["best_iou"][0, 0] == 0.0 and not got["tp_m"][0, 0].any()
        assert got["area_gt"][0, 0] == 0 and not got["inter"][0, :, 0].any()
    if name == "degenerate_boxes":  # inverted, left of the image, below it, zero width, (whole image), NaN x1: empty masks
        assert not got["area_pred"][1, [2, 3, 4, 5, 7]].any() and got["area_pred"][1, 6] > 0
    if name in NEED_TP:
        assert got["tp_m"].any()


def test_wrapper_returns_what_the_entry_point_writes(device):
    c, e = _case("label_slices_differ")
    B, md = len(c["counts"]), c["max_det"]
    bufs = H.NmsBuffers(B, 1, md, device)
    bufs.out.copy_(torch.from_numpy(c["rows"])), bufs.count.copy_(torch.from_numpy(c["counts"]))
    side = torch.cat([torch.from_numpy(c["boxes"]), c["coef"]], 2).to(device).contiguous()
    tp, bi, bl, inter, ap, ag = H.val_mask_match(bufs, c["protos"].to(device).permute(0, 3, 1, 2), side, torch.from_numpy(c["maps"]).to(device),
                                                  torch.from_numpy(c["tcls"]).to(device), torch.from_numpy(c["timg"]).to(device), IOUV, (c["in_hw"][1], c["in_hw"][0]),
                                                  e["l_cap"], want_best=True, want_counts=True)
    got = dict(tp_m=tp.cpu().numpy(), best_iou=bi.cpu().numpy(), best_label=bl.cpu().numpy(), inter=inter.cpu().numpy(), area_pred=ap.cpu().numpy(),
               area_gt=ag.cpu().numpy())
    _check(c, e, got)
    only = H.val_mask_match(bufs, c["protos"].to(device).permute(0, 3, 1, 2), side, torch.from_numpy(c["maps"]).to(device), torch.from_numpy(c["tcls"]).to(device),
                            torch.from_numpy(c["timg"]).to(device), IOUV, (c["in_hw"][1], c["in_hw"][0]), e["l_cap"])
    assert torch.equal(only, tp)
    # a larger l_cap than the largest image needs: the same matches, zero counts behind the labels
    wide = _launch(c, device, l_cap=e["l_cap"] + 3)
    assert np.array_equal(wide["tp_m"], got["tp_m"]) and not wide["inter"][..., e["l_cap"] :].any() and not wide["area_gt"][:, e["l_cap"] :].any()


def test_one_label_above_the_cap_is_refused(device):
    c, e = _case("one_image")
    bufs = H.NmsBuffers(1, 1, c["max_det"], device)
    bufs.out.copy_(torch.from_numpy(c["rows"])), bufs.count.copy_(torch.from_numpy(c["counts"]))
    side = torch.cat([torch.from_numpy(c["boxes"]), c["coef"]], 2).to(device).contiguous()
    args = (bufs, c["protos"].to(device).permute(0, 3, 1, 2), side, torch.from_numpy(c["maps"]).to(device), torch.from_numpy(c["tcls"]).to(device),
            torch.from_numpy(c["timg"]).to(device), IOUV, (32, 32))
    assert L.VAL_MASK_MAX_LABELS == 1024
    with pytest.raises(NotImplementedError, match="1024"):
        H.val_mask_match(*args, L.VAL_MASK_MAX_LABELS + 1)
    assert torch.equal(H.val_mask_match(*args, L.VAL_MASK_MAX_LABELS).cpu(), torch.from_numpy(e["tp_m"].astype(np.uint8)))  # the cap itself runs


def test_exact_tie_goes_to_the_lower_label(device):
    """Two one-pixel labels of one class under a two-pixel mask: both IoUs are exactly 0.5; best is the lower position, which then serves
    the higher-ranked of two identical detections only (the restated rule; the reference's order on such a tie is not defined)."""
    c = case_inputs(5, grid=(8, 8), ratio=1, in_hw=(32, 32), max_det=4, counts=[2], n_labels=[2], one_pixel_labels=True, nc=1)
    c["protos"] = torch.ones_like(c["protos"])
    c["coef"] = torch.ones_like(c["coef"])
    c["boxes"][0, :2] = [-2.0, -2.0, 7.8, 3.8]  # proto pixels (0, 0) and (0, 1)
    c["rows"][0, :2, :4] = c["boxes"][0, :2]
    e = case_expected(c)
    assert e["tie"] and e["unsure"] == 0 and e["area_pred"][0, :2].tolist() == [2, 2] and e["iou"][0].tolist() == [[0.5, 0.5], [0.5, 0.5]]
    got = _launch(c, device)
    _check(c, e, got)
    assert got["best_label"][0, :2].tolist() == [0, 0] and got["tp_m"][0, 0].tolist() == [1] + [0] * 9 and not got["tp_m"][0, 1].any()


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g():
    return golden("segval.npz")


def _bits(g, key, shape):
    return np.unpackbits(g[key])[: int(np.prod(shape))].reshape(shape).astype(bool)


def _yolo_and_data(g, tag):
    m = meta(g, tag)
    y = YOLO(m["yaml"].replace("yolov8-", f"yolov8{m['scale']}-"))
    y.model = SegmentationModel(dict(load_yaml(m["yaml"], m["scale"], m["nc"])), nc=m["nc"], verbose=False)
    y.model.load_state_dict(O.seeded_state_dict(y.model.state_dict(), m["seed"], cls_bias=m["cls_bias"]))
    img = torch.randint(0, 256, m["shape"], generator=torch.Generator().manual_seed(m["seed"]), dtype=torch.uint8)
    data = dict(img=img, batch_idx=torch.from_numpy(g[f"{tag}__batch_idx"]), cls=torch.from_numpy(g[f"{tag}__cls"]).view(-1, 1),
                bboxes=torch.from_numpy(g[f"{tag}__bboxes"]), masks=torch.from_numpy(g[f"{tag}__maps"]))
    return y, m, data


def _val(y, data, m, kept, **kw):
    def make(args):
        v = SegmentationValidator(args)
        kept.append(v)
        return v

    return y.val(validator=make, data=data, batch=m["batch"], iou=0.7, device=0, **kw)


@pytest.mark.parametrize("dtype", ["fp32", None], ids=["f32", "split"])
@pytest.mark.parametrize("tag", ["sv3", "svp2"])
def test_val_end_to_end_against_the_reference(g, tag, dtype, device):
    y, m, data = _yolo_and_data(g, tag)
    n = m["shape"][0]
    kept = []
    kw = dict(dtype=dtype) if dtype else {}
    dev = _val(y, data, m, kept, device_match=True, **kw)
    assert y.metrics is dev and list(dev) == list(SegmentationValidator().metrics.keys) + ["fitness"] and not any(k.startswith("val/") for k in dev)
    host = _val(y, data, m, kept, device_match=False, **kw)
    ref = dict(zip([str(k) for k in g[f"{tag}__result_keys"]], g[f"{tag}__results"]))
    print(tag, dtype or "split", "device", dev, "host", host, "reference", {k: round(float(v), 5) for k, v in ref.items()})
    # per image: tp / tp_m against the recorded matrices wherever the kept rows are the reference's
    vd = kept[0]
    counts, rows_ref = vd.last_counts, g[f"{tag}__rows"]
    tp_ref, tpm_ref = _bits(g, f"{tag}__tp", (n, 300, 10)), _bits(g, f"{tag}__tp_m", (n, 300, 10))
    st = {k: np.concatenate(v, 0) for k, v in vd.last_stats.items()}
    same, o = 0, 0
    for i in range(n):
        k = int(counts[i])
        conf, cls = st["conf"][o : o + k], st["pred_cls"][o : o + k]
        if k == int(g[f"{tag}__counts"][i]) and np.array_equal(cls, rows_ref[i, :k, 5]) and np.abs(conf - rows_ref[i, :k, 4]).max() <= 1e-4:
            same += 1
            assert np.array_equal(st["tp"][o : o + k], tp_ref[i, :k]), f"image {i}: box tp differs from the reference's"
            assert np.array_equal(st["tp_m"][o : o + k], tpm_ref[i, :k]), f"image {i}: mask tp_m differs from the reference's"
        o += k
    print(tag, dtype or "split", f"images whose kept rows are the reference's: {same} of {n}")
    assert same >= 1
    assert dev == host, "device_match=True and False disagree"
    worst = {k: abs(dev[k] - ref[k]) for k in ref}
    print(tag, dtype or "split", "distance to the reference's results_dict", worst)
    assert max(worst.values()) <= 1e-4 + 5e-6, worst  # (5e-6: the dict is rounded to 5 digits)


def test_val_half_runs(g, device):
    y, m, data = _yolo_and_data(g, "svp2")
    out = _val(y, data, m, [], half=True)
    print("svp2 half=True", out)
    assert y.metrics is out and all(np.isfinite(v) for v in out.values()) and len(out) == 9
