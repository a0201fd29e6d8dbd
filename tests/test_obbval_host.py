"""Oriented-box validation without a GPU: ``OBBMetrics``, the host arithmetic of ``OBBValidator`` against the reference's recorded ``tp``, the
dataset refusal of ``YOLO.val``, the two new entry points' argument checks, and the conditions under which tests/golden/obbval.npz's cases
were accepted (tools/make_obbval_golden.py), re-derived here from the stored seeds with this package's restatements of ``batch_probiou``
and ``match_predictions``."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from drone_yolo_amd import YOLO
from drone_yolo_amd.engine.validator import OBBValidator, obb_labels
from drone_yolo_amd.utils.metrics import DetMetrics, OBBMetrics, batch_probiou, match_predictions
from tests import _obbval_util as V
from tests._util import golden, meta

MATCH_NAMES = list(V.MATCH_CASES) + ["single_cls"]


@pytest.fixture(scope="module")
def g():
    return golden("obbval.npz")


def _probiou32(a, b):
    return batch_probiou(np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)).numpy()


def _match32(pcls, tcls, iou):
    return match_predictions(np.asarray(pcls, np.float32), np.asarray(tcls, np.float32), np.asarray(iou, np.float32), V.IOUV)


def unpack(g, key, shape):
    return np.unpackbits(g[key])[: int(np.prod(shape))].reshape(shape).astype(bool)


@functools.lru_cache(maxsize=None)
def match_case(name):
    """(inputs, float64 / fp32 evaluation) of a kernel-free case at its stored seed: computed once, shared, not modified."""
    g = golden("obbval.npz")
    c = V.match_inputs(name, int(g[f"m_{name}__seed"]))
    return c, V.match_evaluate(c, _probiou32, _match32, fixed=tuple(float(v) for v in g[f"m_{name}__margin"]))


def test_obbmetrics_carries_the_reference_keys():
    m = OBBMetrics()
    assert isinstance(m, DetMetrics) and type(m).__name__ == "OBBMetrics"
    assert m.keys == ("metrics/precision(B)", "metrics/recall(B)", "metrics/mAP50(B)", "metrics/mAP50-95(B)")
    assert list(m.results_dict) == list(m.keys) + ["fitness"] and all(v == 0.0 for v in m.results_dict.values())
    v = OBBValidator(dict(conf=None, iou=0.6, max_det=50, single_cls=True))
    assert isinstance(v.metrics, OBBMetrics) and v.conf == 0.001 and v.agnostic and v.device_match and v.last_stats is None


@pytest.mark.parametrize("name", MATCH_NAMES)
def test_match_fixture_conditions_hold_at_the_stored_seed(g, name):
    c, e = match_case(name)
    B, md = len(c["counts"]), c["max_det"]
    assert e["ok"], f"{name}: the acceptance conditions do not hold at seed {int(g[f'm_{name}__seed'])}"
    M, M_top = (float(v) for v in g[f"m_{name}__margin"])
    # (judged with the recorded margins; what this CPU's fp32 measures stays within a factor of two of them)
    assert e["M_meas"] <= 2 * M and e["M_top_meas"] <= 2 * M_top and (name != "val300" or e["M_meas"] >= M / 2)
    assert 0 < M < 1e-3 and M_top < 2e-2
    rec = unpack(g, f"m_{name}__tp", (B, md, 10))
    assert np.array_equal(rec, e["tp32"]) and np.array_equal(rec, e["tp64"])
    assert np.array_equal(g[f"m_{name}__best_label"], e["best_label64"]) and np.allclose(g[f"m_{name}__best_iou"], e["best_iou64"], rtol=0, atol=1e-12)
    assert not np.isnan(e["best_iou64"]).any()
    for i, cnt in enumerate(c["counts"]):
        assert not rec[i, cnt:].any()


def test_match_cases_are_what_they_are_for(g):
    c, e = match_case("few")
    assert c["counts"].tolist() == [0, 1, 5] and np.bincount(c["timg"], minlength=3).tolist() == [3, 0, 4] and not np.all(np.diff(c["timg"]) >= 0)
    c, e = match_case("rank")  # the higher-ranked detection has the lower IoU and the same best label
    b0, b1 = e["best_iou64"][0, :2]
    assert e["best_label64"][0, 0] == e["best_label64"][0, 1] == 0 and 0.5 < b0 < b1
    both = V.IOUV <= b0
    assert both.sum() >= 2 and (V.IOUV[~both] <= b1).sum() >= 2
    assert e["tp64"][0, 0].tolist() == both.tolist(), "the higher-ranked detection takes the label at the thresholds it reaches"
    assert e["tp64"][0, 1].tolist() == (~both & (V.IOUV <= b1)).tolist(), "the later one loses it there and wins it at the thresholds only it reaches"
    c, e = match_case("step")
    assert len(c["tbox"]) == 530 and c["max_det"] == 16
    c, e = match_case("stride")
    assert c["counts"].tolist() == [520, 3] and c["max_det"] == 520
    c, e = match_case("clip")
    W, H = c["clip"]
    r = c["rows"][0, : c["counts"][0]]
    assert (r[:, 0] < 0).any() or (r[:, 1] > H).any() or (r[:, 2] > W).any() or (r[:, 3] > H).any()
    assert (c["tbox"][:, 2] == W).any() and (c["tbox"][:, 3] == H).any() and (c["tbox"][:, 0] == 0).any() and (c["tbox"][:, 1] == H).any()
    c, e = match_case("angles")
    th = np.concatenate((c["rows"][0, : c["counts"][0], 4], c["tbox"][:, 4]))
    assert (th >= np.pi / 2).any() and (th < 0).any() and th.min() > -np.pi / 4 - 1.0 and th.max() < 3 * np.pi / 4 + 1.0
    swap = V.MATCH_CASES["angles"]["swap"]
    for k in range(swap):  # a label equal to its detection up to (w, h, theta) <-> (h, w, theta + pi / 2) scores as the same box
        l = c["tbox"][e["best_label64"][0, k]]
        d = c["rows"][0, k]
        assert np.allclose(l[:2], d[:2]) and np.allclose(l[2:4], d[[3, 2]]) and abs(abs(l[4] - d[4]) - np.pi / 2) < 1e-5
        same_way = V.probiou64(l[None], l[None])[0, 0]
        assert e["best_iou64"][0, k] > 0.999 and abs(e["best_iou64"][0, k] - same_way) < 1e-6
    c, e = match_case("degenerate")
    cnt = c["counts"][0]
    assert (c["tbox"][:, 2] == 0).sum() == 1 and c["rows"][0, 0, 3] == 0
    zl = int(np.flatnonzero(c["tbox"][:, 2] == 0)[0])
    assert not e["tp64"][0, 0].any(), "the zero-height detection is never matched"
    assert not (e["tp64"][0, :cnt].any(1) & (e["best_label64"][0, :cnt] == zl)).any(), "the zero-width label is never matched"
    c, e = match_case("single_cls")
    assert c["single_cls"] and not c["tcls"].any() and e["tp64"].any() and np.array_equal(c["rows"], match_case("few")[0]["rows"])


@functools.lru_cache(maxsize=None)
def seedless_case(name):
    """(inputs, float64 tp, float64 best label) of the full-stage / layout-bound cases: computed once, shared, not modified."""
    c = dict(full_stage=V.full_stage_case, bound=V.bound_case)[name]()
    tp, best, scores = V.expect64(c)
    assert ((scores > 0.99) | (scores < 0.01)).all(), "every threshold is decided by a margin thousands of times the recorded M"
    return c, tp, best


def test_full_stage_and_bound_cases_are_what_they_are_for():
    c, tp, best = seedless_case("full_stage")
    assert len(c["tbox"]) == 257 and not c["timg"].any() and (c["tcls"] == 1).all() and c["counts"].tolist() == [4] and c["max_det"] == 4
    d = c["tbox"][:, None, :2] - c["tbox"][None, :, :2]
    assert np.sqrt((d ** 2).sum(-1))[~np.eye(257, dtype=bool)].min() >= 60 and len(np.unique(c["tbox"][:, 4])) > 3
    assert best.tolist() == [0, 255, 256, 256] and tp[:3].all() and not tp[3].any()
    c, tp, best = seedless_case("bound")
    assert c["max_det"] == 4096 and c["counts"].tolist() == [4096] and len(c["tbox"]) == 5 and not np.isin(c["rows"][0, 5:, 6], c["tcls"]).any()
    assert best[:5].tolist() == [0, 1, 2, 3, 4] and tp[:5].all() and not tp[5:].any()
    v = OBBValidator()
    for name in ("full_stage", "bound"):  # the validator's host arithmetic (fp32) gives the same verdicts
        c, tp, _ = seedless_case(name)
        assert np.array_equal(v.host_match(c["rows"][0], c["tbox"], c["tcls"], *c["clip"]), tp)


@pytest.mark.parametrize("name", list(V.NMS_CASES))
def test_nms_fixture_conditions_hold_at_the_stored_seed(g, name):
    counts, anchors, nc, _, kw, _ = V.NMS_CASES[name]
    pred, theta = V.nms_inputs(name, int(g[f"n_{name}__seed"]))
    if not name.startswith("two"):
        assert V.pair_counts(pred, nc) == counts
    else:
        assert (pred[0, 4:, 17] > V.CONF).sum() == 2
    ok, M, kept = V.nms_evaluate(pred, theta, nc, kw, _probiou32, fixed=float(g[f"n_{name}__margin"][0]))
    assert ok and M <= 2 * float(g[f"n_{name}__margin"][0])
    rec_n = [int(k) for k in g[f"n_{name}__n"]]
    idx, rows, o = g[f"n_{name}__idx"], g[f"n_{name}__rows"], 0
    for b, k in enumerate(rec_n):  # the reference's kept rows are the float64 verdicts' (first max_det of them)
        a, c, _, s = V.ml_sorted_candidates(pred, theta, b, nc, kw)
        keep = kept[b][: kw.get("max_det", 300)]
        assert len(keep) == k and np.array_equal(a[keep].numpy(), idx[o : o + k]) and np.array_equal(c[keep].numpy(), rows[o : o + k, 5].astype(np.int64))
        assert np.array_equal(s[keep].numpy(), rows[o : o + k, 4])
        o += k
    if name == "lds_cap":
        assert anchors < V.U.LDS_CAP < V.pair_counts(pred, nc)[0] and V.pair_counts(pred, nc)[1] < V.U.LDS_CAP
    if name == "two":
        assert rec_n[0] == 2 and idx[:2].tolist() == [17, 17]
    if name == "two_agnostic":
        assert rec_n[0] == 1 and idx[0] == 17 and rows[0, 5] == 0
    if name == "crowd":
        assert rec_n[0] == kw["max_det"] and len(kept[0]) > kw["max_det"]
    if name == "max_nms":
        assert V.pair_counts(pred, nc)[0] > kw["max_nms"]


# ---- the validator's host arithmetic on the recorded rows ------------------------------------------------------------------------------
def e2e_fixture(g, tag):
    m = meta(g, tag)
    n = m["shape"][0]
    counts = g[f"{tag}__counts"]
    rows = np.zeros((n, 300, 7), np.float32)
    rows[:, : g[f"{tag}__rows"].shape[1]] = g[f"{tag}__rows"]
    return m, counts, rows, unpack(g, f"{tag}__tp", (n, 300, 10)), dict(zip((str(k) for k in g[f"{tag}__result_keys"]), g[f"{tag}__results"]))


@pytest.mark.parametrize("tag", list(V.E2E))
def test_host_match_on_recorded_rows_gives_the_reference_tp_and_dict(g, tag):
    m, counts, rows, tp_ref, res_ref = e2e_fixture(g, tag)
    h, w = m["shape"][2:]
    v = OBBValidator(dict(conf=m["conf"], iou=m["iou"]))
    bidx, cls, bboxes = g[f"{tag}__batch_idx"], g[f"{tag}__cls"], torch.from_numpy(g[f"{tag}__bboxes"])
    assert bboxes.shape[1] == 5 and all((bidx == i).any() for i in range(len(counts))), "every image has labels"
    lim = torch.tensor((w, h, w, h), dtype=torch.float32)
    stats = dict(tp=[], conf=[], pred_cls=[], target_cls=[])
    for i, k in enumerate(counts):
        sel = bidx == i
        tbox = obb_labels(bboxes[sel], w, h, lim).numpy()
        assert np.array_equal(tbox[:, 4], bboxes[sel][:, 4].numpy()), "the angle is untouched"
        tp = v.host_match(rows[i, :k], tbox, cls[sel], w, h)
        assert np.array_equal(tp, tp_ref[i, :k]), f"{tag}: image {i}"
        assert np.array_equal(rows[i, :k, 5], g[f"{tag}__conf"][i, :k]) and np.array_equal(rows[i, :k, 6], g[f"{tag}__pred_cls"][i, :k])
        stats["tp"].append(tp), stats["conf"].append(rows[i, :k, 5]), stats["pred_cls"].append(rows[i, :k, 6]), stats["target_cls"].append(cls[sel])
    v.metrics.process(*(np.concatenate(stats[k]) for k in ("tp", "conf", "pred_cls", "target_cls")))
    got = v.metrics.results_dict
    assert set(got) == set(res_ref)
    for k in got:
        assert round(float(got[k]), 5) == round(float(res_ref[k]), 5), (k, got[k], res_ref[k])
    assert tp_ref.any(axis=(1, 2)).all() and 0 < res_ref["metrics/mAP50-95(B)"] < res_ref["metrics/mAP50(B)"]


# ---- YOLO.val ---------------------------------------------------------------------------------------------------------------------------
def test_val_refuses_a_dataset_without_angles_before_any_device_use():
    y = YOLO("yolov8n-obb.yaml")
    data = dict(img=torch.zeros((2, 3, 64, 64), dtype=torch.uint8), batch_idx=torch.tensor([0.0, 1.0]), cls=torch.zeros((2, 1)),
                bboxes=torch.tensor([[0.5, 0.5, 0.2, 0.2], [0.4, 0.4, 0.1, 0.3]]))
    for d in (data, "synthetic:4"):
        with pytest.raises(NotImplementedError, match=r"val: an oriented-box model needs .*\(M, 5\) xywhr"):
            y.val(data=d, device=0)
    assert y.predictor is None and getattr(y, "metrics", None) is None
    assert all(p.device.type == "cpu" for p in y.model.parameters())
    for call in (lambda: y.train(data="synthetic:4"), lambda: y.track(torch.zeros(1, 3, 64, 64)), lambda: y.predict(torch.zeros(1, 3, 64, 64), tile=64),
                 lambda: y.predict(torch.zeros(1, 3, 64, 64), augment=True)):
        with pytest.raises(NotImplementedError):
            call()
    with pytest.raises(ValueError, match="data"):
        y.val()


def test_loader_passes_five_column_boxes_through():
    from drone_yolo_amd.engine.trainer import TensorLoader, load_dataset

    data = dict(img=torch.zeros((3, 3, 32, 32), dtype=torch.uint8), batch_idx=torch.tensor([2.0, 0.0, 2.0]), cls=torch.tensor([[1.0], [2.0], [0.0]]),
                bboxes=torch.tensor([[0.5, 0.5, 0.2, 0.2, 0.3], [0.4, 0.4, 0.1, 0.3, -0.5], [0.1, 0.2, 0.3, 0.4, 1.9]]))
    d = load_dataset(data, 32, 3, 0)
    batches = list(TensorLoader(d, 2, 0, 1, shuffle=False))
    assert [tuple(b["bboxes"].shape) for b in batches] == [(1, 5), (2, 5)]
    assert torch.equal(batches[0]["bboxes"], data["bboxes"][1:2]) and torch.equal(batches[1]["bboxes"], data["bboxes"][[0, 2]]) and batches[1]["batch_idx"].tolist() == [0.0, 0.0]


# ---- the C interface without a device -------------------------------------------------------------------------------------------------
def test_new_entry_points_validate_without_gpu(tmp_path):
    import os
    import subprocess

    from drone_yolo_amd import _lib as L
    from tests._util import ROOT

    h = L.lib()
    assert h.dy_nms_rotated_ml(ctypes.byref(L.NmsDesc()), None, None) == -1 and b"dy_nms_rotated_ml" in h.dy_last_error_string()
    buf = ctypes.cast((ctypes.c_float * 64)(), ctypes.c_void_p)
    d = L.NmsDesc()
    d.pred = d.out = d.out_count = d.workspace = buf
    d.batch, d.nc, d.anchors, d.conf_thres, d.iou_thres, d.max_det, d.max_nms = 1, 3, 100, 0.001, 0.7, 300, 30000
    need = h.dy_nms_rotated_ml_workspace_bytes(1, 100, 3)
    assert need == h.dy_nms_workspace_bytes(1, 300) + 1 * 5 * 300 * 4  # (the dy_nms workspace of 300 candidates is a multiple of 256 bytes)
    assert h.dy_nms_rotated_ml_workspace_bytes(1, 100, 1) == h.dy_nms_rotated_workspace_bytes(1, 100)
    assert h.dy_nms_rotated_ml_workspace_bytes(0, 100, 3) == -1 and h.dy_nms_rotated_ml_workspace_bytes(1, 100, 0) == -1 and h.dy_nms_rotated_ml_workspace_bytes(1, 1 << 20, 1 << 10) == -1
    d.workspace_bytes = h.dy_nms_rotated_workspace_bytes(1, 100)  # the single-label size: too small for (anchor, class) pairs
    assert h.dy_nms_rotated_ml(ctypes.byref(d), buf, None) == -4 and b"dy_nms_rotated_ml: workspace" in h.dy_last_error_string()  # DY_ERR_WORKSPACE
    d.workspace_bytes = need - 1
    assert h.dy_nms_rotated_ml(ctypes.byref(d), buf, None) == -4
    d.workspace_bytes, d.prefiltered = need, 1
    assert h.dy_nms_rotated_ml(ctypes.byref(d), buf, None) == -2 and b"dy_nms_rotated_ml" in h.dy_last_error_string()  # DY_ERR_UNSUPPORTED
    d.prefiltered, d.max_det = 0, 5000
    assert h.dy_nms_rotated_ml(ctypes.byref(d), buf, None) == -1
    d.max_det, d.multi_label = 300, 1
    assert h.dy_nms_rotated(ctypes.byref(d), buf, None) == -2, "dy_nms_rotated keeps refusing multi_label"

    m = L.ValMatchRotatedDesc()
    assert h.dy_val_match_rotated(ctypes.byref(m), None) == -1 and b"dy_val_match_rotated" in h.dy_last_error_string()
    assert h.dy_val_match_rotated(None, None) == -1
    thr = (ctypes.c_float * 10)(*V.IOUV.tolist())
    m.rows = m.counts = m.tp = buf
    m.iouv, m.batch, m.max_det, m.n_iouv = thr, 1, 4097, 10
    assert h.dy_val_match_rotated(ctypes.byref(m), None) == -1 and b"max_det" in h.dy_last_error_string()
    m.max_det, m.n_iouv = 300, 17
    assert h.dy_val_match_rotated(ctypes.byref(m), None) == -1 and b"n_iouv" in h.dy_last_error_string()
    m.n_iouv, m.n_labels = 10, 3
    assert h.dy_val_match_rotated(ctypes.byref(m), None) == -1 and b"label pointer" in h.dy_last_error_string()
    m.tbox = m.tcls = m.timg = ctypes.c_void_p(buf.value + 4)
    assert h.dy_val_match_rotated(ctypes.byref(m), None) == -1 and b"16-byte" in h.dy_last_error_string()
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include "dyolo.h"\nint main(){printf("%zu %zu\\n", sizeof(dy_val_match_rotated_desc), sizeof(dy_val_match_desc));return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "s")])
    sizes = [int(v) for v in subprocess.check_output([str(tmp_path / "s")]).split()]
    assert sizes == [ctypes.sizeof(L.ValMatchRotatedDesc), ctypes.sizeof(L.ValMatchDesc)]
