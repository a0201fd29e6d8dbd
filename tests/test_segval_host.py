"""CPU: the segmentation validator without a device — the 2 x 2 replication claim behind the ratio-2 label map, the host pieces of
``device_match=False`` and ``SegmentMetrics`` against the REAL reference's recorded results (tests/golden/segval.npz,
tools/make_segval_golden.py), the restated match rule against ``match_predictions``, the mutations the comparison must flag, the refusals
and the C-ABI checks of ``dy_val_mask_match``."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from drone_yolo_amd import YOLO
from drone_yolo_amd import hip_ops as H
from drone_yolo_amd.engine.trainer import TensorLoader
from drone_yolo_amd.engine.validator import check_mask_grids, host_gt_masks, host_mask_iou, host_pred_masks
from drone_yolo_amd.utils.metrics import SegmentMetrics, match_predictions
from tests._segval_util import IOUV, case_expected, case_inputs, expand_map, has_tie, iou32, match_rule
from tests._util import ROOT, golden, meta

MI_TAGS = ["mi_r1", "mi_r2"]
SV_TAGS = ["sv3", "svp2"]


@pytest.fixture(scope="module")
def g():
    return golden("segval.npz")


def _bits(g, key, shape):
    return np.unpackbits(g[key])[: int(np.prod(shape))].reshape(shape).astype(bool)


# ---- the replication claim -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(1, 1), (3, 5), (8, 8)])
def test_bilinear_2x_of_a_one_hot_mask_is_its_2x2_replication(hw):
    """F.interpolate(onehot, 2x, bilinear, align_corners=False).gt(0.5) == the 2 x 2 replication of the label's map pixels, for every label:
    labels on the border, scattered single pixels, and a label that owns no pixel."""
    gh, gw = hw
    rng = np.random.default_rng(gh * 16 + gw)
    for trial in range(8):
        nl = 1 + trial % 4
        gmap = rng.integers(0, nl + 1, (gh, gw))  # label nl + 1 never appears: it owns no pixel
        gmap[0, :] = rng.integers(0, nl + 1, gw)
        if trial == 0:
            gmap[:] = 1  # one label owns everything, borders included
        onehot = torch.where(torch.from_numpy(gmap)[None].repeat(nl + 1, 1, 1) == torch.arange(nl + 1).view(-1, 1, 1) + 1, 1.0, 0.0)
        up = F.interpolate(onehot[None], (2 * gh, 2 * gw), mode="bilinear", align_corners=False)[0].gt_(0.5).numpy().astype(bool)
        rep = expand_map(gmap, 2)
        for l in range(nl + 1):
            assert np.array_equal(up[l], rep == l + 1), (hw, trial, l)
        assert not up[nl].any()
        # and the host piece of device_match=False takes exactly that route
        assert np.array_equal(host_gt_masks(torch.from_numpy(gmap), nl + 1, (2 * gh, 2 * gw)).numpy().astype(bool), up)


# ---- the host path against the reference's recorded results ---------------------------------------------------------------------------
def _host_chain(c, b):
    """The pieces of ``device_match=False`` on image b of a case -> inter (nl, k), area_pred, area_gt, iou, tp_m."""
    k, nl = int(c["counts"][b]), c["n_labels"][b]
    off = sum(c["n_labels"][:b])
    pm = host_pred_masks(c["protos"][b].permute(2, 0, 1).contiguous(), c["coef"][b, :k], torch.from_numpy(c["boxes"][b, :k]), c["in_hw"])
    gt = host_gt_masks(torch.from_numpy(c["maps"][b]), nl, c["grid"])
    iou = host_mask_iou(gt, pm)
    px = c["grid"][0] * c["grid"][1]
    g2, p2 = gt.reshape(nl, px).numpy(), pm.reshape(k, px).numpy()
    tp = match_predictions(c["rows"][b, :k, 5], c["tcls"][off : off + nl], iou, IOUV) if k and nl else np.zeros((k, 10), bool)
    return (g2 @ p2.T).astype(np.int64), p2.sum(1).astype(np.int64), g2.sum(1).astype(np.int64), iou, tp


@pytest.mark.parametrize("tag", MI_TAGS)
def test_host_pieces_reproduce_the_reference_mask_iou_cases(g, tag):
    m = meta(g, tag)
    c = case_inputs(**m)
    B, md = len(c["counts"]), c["max_det"]
    ref_tp = _bits(g, f"{tag}__tp_m", (B, md, 10))
    assert int(g[f"{tag}__unsure"]) == 0 and np.array_equal(g[f"{tag}__inter"], g[f"{tag}__inter64"])
    e = case_expected(c)  # the float64 evaluation at run time agrees with the recorded one and with the reference
    assert np.array_equal(e["inter"], g[f"{tag}__inter"]) and np.array_equal(e["area_pred"], g[f"{tag}__area_pred"])
    assert np.array_equal(e["area_gt"], g[f"{tag}__area_gt"]) and np.array_equal(e["tp_m"], ref_tp)
    assert np.array_equal(e["best_iou"], g[f"{tag}__best_iou"]) and np.array_equal(e["best_label"], g[f"{tag}__best_label"])
    ious = []
    for b in range(B):
        k, nl = int(c["counts"][b]), c["n_labels"][b]
        inter, ap, ag, iou, tp = _host_chain(c, b)
        assert np.array_equal(inter.T, g[f"{tag}__inter"][b, :k, :nl]) and np.array_equal(ap, g[f"{tag}__area_pred"][b, :k])
        assert np.array_equal(ag, g[f"{tag}__area_gt"][b, :nl])
        assert np.array_equal(tp, ref_tp[b, :k]) and not ref_tp[b, k:].any()
        assert np.array_equal(iou, iou32(inter, ag, ap))  # the fp32 expression on the counts, bit for bit
        ious.append(iou.ravel())
    assert np.array_equal(np.concatenate(ious).astype(np.float32), g[f"{tag}__iou"])
    assert ref_tp.sum() >= 2


@pytest.mark.parametrize("tag", SV_TAGS)
def test_segment_metrics_reproduce_the_reference_results_dict(g, tag):
    """SegmentMetrics on the reference validator's own statistics -> its results_dict to 1e-12 (the bar of
    test_validation_metrics_match_the_reference_functions)."""
    m = meta(g, tag)
    n = m["shape"][0]
    counts = g[f"{tag}__counts"]
    keep = np.arange(300)[None, :] < counts[:, None]
    tp, tp_m = _bits(g, f"{tag}__tp", (n, 300, 10)), _bits(g, f"{tag}__tp_m", (n, 300, 10))
    rows = g[f"{tag}__rows"]
    sm = SegmentMetrics()
    sm.process(tp[keep], tp_m[keep], rows[keep][:, 4], rows[keep][:, 5], g[f"{tag}__cls"])
    got = sm.results_dict
    ref = dict(zip([str(k) for k in g[f"{tag}__result_keys"]], g[f"{tag}__results"]))
    assert list(got) == list(SegmentMetrics.keys) + ["fitness"] and set(got) == set(ref)
    assert SegmentMetrics.keys[:4] == ("metrics/precision(B)", "metrics/recall(B)", "metrics/mAP50(B)", "metrics/mAP50-95(B)")
    assert SegmentMetrics.keys[4:] == ("metrics/precision(M)", "metrics/recall(M)", "metrics/mAP50(M)", "metrics/mAP50-95(M)")
    for k in ref:
        assert abs(got[k] - ref[k]) <= 1e-12, (k, got[k], ref[k])
    assert abs(got["fitness"] - (sm.box.fitness + sm.seg.fitness)) <= 1e-15 and got["metrics/mAP50(M)"] > 0


# ---- the match rule -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", MI_TAGS)
def test_restated_rule_equals_match_predictions_on_the_golden_iou(g, tag):
    m = meta(g, tag)
    c = case_inputs(**m)
    flat, o, off = g[f"{tag}__iou"], 0, 0
    ref_tp = _bits(g, f"{tag}__tp_m", (len(c["counts"]), c["max_det"], 10))
    for b, k in enumerate(c["counts"]):
        nl = c["n_labels"][b]
        iou = flat[o : o + nl * k].reshape(nl, k)
        o += nl * k
        pc, tc = c["rows"][b, :k, 5], c["tcls"][off : off + nl]
        off += nl
        best, biou, tp = match_rule(pc, tc, iou)
        assert not has_tie(pc, tc, iou)
        if k and nl:
            assert np.array_equal(tp, match_predictions(pc, tc, iou, IOUV)) and np.array_equal(tp, ref_tp[b, :k])
        else:
            assert not tp.any() and (best == -1).all()
    # an exact tie: the restated rule gives the lower label, and a label serves the higher-ranked detection only
    iou = np.array([[0.8, 0.8], [0.8, 0.6]], np.float32)
    best, biou, tp = match_rule(np.zeros(2), np.zeros(2), iou)
    assert best.tolist() == [0, 0] and tp[0, :7].all() and not tp[1].any()


# ---- mutants -------------------------------------------------------------------------------------------------------------------------
def test_comparison_flags_each_mutation():
    """What a wrong kernel would produce differs from the float64 evaluation in the pinned quantities."""
    c = case_inputs(3001, grid=(40, 52), ratio=2, in_hw=(80, 104), max_det=8, counts=[6, 7], n_labels=[5, 4], nc=3)
    e = case_expected(c)

    def differs(mut, keys=("inter", "area_pred", "area_gt", "best_iou", "best_label", "tp_m")):
        return [k for k in keys if not np.array_equal(e[k], mut[k], equal_nan=True)]

    assert "area_pred" in differs(case_expected(c, crop_shift=1)) and "inter" in differs(case_expected(c, crop_shift=1))  # a crop edge moved by one proto pixel
    shifted = differs(case_expected(c, no_shift=True))  # ratio-2 labels read at [y, x]
    assert "inter" in shifted and "area_gt" in shifted
    dropped = differs(case_expected(c, drop_class=True))  # no class test
    assert "best_iou" in dropped or "best_label" in dropped
    assert not differs(case_expected(c, drop_class=True), ("inter", "area_pred", "area_gt"))
    # the missing 1e-7 shows on the empty-against-empty pair: 0 / 0
    z = case_inputs(11, grid=(8, 8), ratio=1, in_hw=(32, 32), max_det=4, counts=[2], n_labels=[2], nc=1, empty_label=True, empty_pred=True)
    ez = case_expected(z)
    assert ez["area_pred"][0, 0] == 0 and ez["area_gt"][0, 0] == 0 and ez["iou"][0][0, 0] == 0.0 and not ez["tp_m"][0, 0].any()
    with np.errstate(invalid="ignore"):
        assert np.isnan(case_expected(z, no_eps=True)["iou"][0][0, 0])
    assert iou32(np.zeros((1, 1)), np.zeros(1), np.zeros(1))[0, 0] == 0.0


# ---- refusals and layout ------------------------------------------------------------------------------------------------------------
def _tiny_dataset(n=2, s=64, with_masks=True, map_hw=(16, 16), dtype=torch.uint8):
    d = dict(img=torch.zeros(n, 3, s, s, dtype=torch.uint8), batch_idx=torch.tensor([0.0, 0.0, 1.0]), cls=torch.tensor([[1.0], [2.0], [0.0]]),
             bboxes=torch.tensor([[0.5, 0.5, 0.2, 0.2], [0.3, 0.3, 0.1, 0.1], [0.6, 0.6, 0.3, 0.3]]))
    if with_masks:
        d["masks"] = torch.zeros(n, *map_hw, dtype=dtype)
    return d


def test_dataset_without_masks_is_refused_before_any_device_use():
    y = YOLO("yolov8n-seg.yaml")
    for data in ("synthetic:4", _tiny_dataset(with_masks=False)):
        with pytest.raises(NotImplementedError, match="val.*masks"):
            y.val(data=data, imgsz=64)
        assert y.predictor is None and y.trainer is None and not hasattr(y, "metrics")
    assert next(y.model.parameters()).device.type == "cpu"
    # one binary mask per label (overlap_mask=False: a float (L, h, w) stack) is not built
    bad = _tiny_dataset()
    bad["masks"] = torch.zeros(3, 16, 16)
    with pytest.raises(NotImplementedError, match="val.*overlap"):
        y.val(data=bad)
    with pytest.raises(NotImplementedError, match="train"):
        y.model.init_criterion()


def test_tensor_loader_yields_masks_only_when_the_dataset_has_them():
    d = _tiny_dataset()
    d["masks"][1, 2, 3] = 1
    batches = list(TensorLoader(d, 1, 0, 1, shuffle=False))
    assert [set(b) for b in batches] == [{"img", "batch_idx", "cls", "bboxes", "masks"}] * 2
    assert torch.equal(batches[1]["masks"], d["masks"][1:2]) and batches[0]["cls"].view(-1).tolist() == [1.0, 2.0]
    plain = list(TensorLoader(_tiny_dataset(with_masks=False), 2, 0, 1, shuffle=False))
    assert set(plain[0]) == {"img", "batch_idx", "cls", "bboxes"}


def test_grid_relations():
    assert check_mask_grids((24, 24), (24, 24)) == 1 and check_mask_grids((32, 48), (16, 24)) == 2
    for proto, gmap in (((48, 48), (16, 16)), ((32, 48), (16, 48)), ((16, 24), (32, 48))):
        with pytest.raises(ValueError, match="twice"):
            check_mask_grids(proto, gmap)
    assert H.val_mask_match_check((32, 48), (16, 24), 300, 10) == 2
    with pytest.raises(ValueError, match="twice"):
        H.val_mask_match_check((48, 48), (16, 16), 4, 10)  # ratio 3
    with pytest.raises(ValueError, match="2\\^24"):
        H.val_mask_match_check((4100, 4100), (4100, 4100), 4, 10)
    with pytest.raises(NotImplementedError, match="1024"):
        H.val_mask_match_check((8, 8), (8, 8), 1025, 10)


def test_val_mask_match_descriptor_validates_without_gpu():
    import drone_yolo_amd._lib as L

    h = L.lib()
    buf = (ctypes.c_float * 1024)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    thr = (ctypes.c_float * 10)(*np.linspace(0.5, 0.95, 10))
    assert h.dy_val_mask_match(None, None) == -1
    assert h.dy_val_mask_match(ctypes.byref(L.ValMaskMatchDesc()), None) == -1 and b"null" in h.dy_last_error_string()

    def desc(**kw):
        d = L.ValMaskMatchDesc()
        d.protos = d.side = d.rows = d.counts = d.map = d.tcls = d.loff = d.tp_m = d.best_iou = d.best_label = d.area_gt = p
        d.iouv = thr
        d.batch, d.max_det, d.nm, d.mh, d.mw, d.ld_p, d.gh, d.gw, d.map_dtype, d.n_labels, d.l_cap, d.n_iouv = 1, 8, 32, 8, 8, 32, 8, 8, L.DY_MAP_U8, 2, 2, 10
        d.in_w, d.in_h = 32, 32
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    for kw, rc, word in ((dict(nm=16), -2, b"nm = 32"), (dict(gh=3, gw=3), -1, b"twice"), (dict(gh=4, gw=8), -1, b"twice"), (dict(l_cap=1025), -2, b"1024"),
                         (dict(mh=4100, mw=4100, gh=4100, gw=4100), -1, b"2^24"), (dict(n_iouv=17), -1, b"n_iouv"), (dict(map_dtype=5), -1, b"map_dtype"),
                         (dict(max_det=5000), -1, b"max_det"), (dict(ld_p=30), -1, b"128-byte"), (dict(in_w=0), -1, b"input size"), (dict(area_gt=None), -1, b"null")):
        assert h.dy_val_mask_match(ctypes.byref(desc(**kw)), None) == rc, kw
        assert word in h.dy_last_error_string(), (kw, h.dy_last_error_string())


def test_val_mask_match_struct_layout_matches_the_header(tmp_path):
    import drone_yolo_amd._lib as L

    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dyolo.h"\nint main(){printf("%zu %zu %zu %zu\\n", sizeof(dy_val_mask_match_desc), '
                   "offsetof(dy_val_mask_match_desc, batch), offsetof(dy_val_mask_match_desc, in_w), offsetof(dy_val_mask_match_desc, tp_m));return 0;}\n")
    exe = tmp_path / "s"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    D = L.ValMaskMatchDesc
    assert sizes == [ctypes.sizeof(D), D.batch.offset, D.in_w.offset, D.tp_m.offset]
    assert L.DY_MAP_U8 == 0 and L.DY_MAP_I32 == 1
