"""CPU: the oriented-box task's construction, refusals, host helpers and fixtures (tests/golden/obb.npz, tools/make_obb_golden.py)."""
import numpy as np
import pytest
import torch

import drone_yolo_amd as D
from drone_yolo_amd import YOLO
from drone_yolo_amd.engine.results import OBB, Results
from drone_yolo_amd.nn import modules as M
from drone_yolo_amd.nn.tasks import DetectionModel, OBBModel, guess_model_task
from drone_yolo_amd.utils import metrics, ops
from tests import _obb_util as U
from tests._util import golden, load_yaml, meta


@pytest.fixture(scope="module")
def g():
    return golden("obb.npz")


# ---- construction and task ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tag", [("yolov8n-obb.yaml", "obb3n64x96"), ("yolov8n-p2-repvgg-obb.yaml", "obbn64x96")])
def test_yolo_builds_an_obb_model_with_the_reference_state_dict(g, name, tag):
    y = YOLO(name)
    assert y.task == "obb" and type(y.model) is OBBModel and isinstance(y.model.model[-1], M.OBB) and y.overrides["task"] == "obb"
    m = meta(g, tag)
    model = OBBModel(dict(load_yaml(m["yaml"], m["scale"], m["nc"])), nc=m["nc"], verbose=False)
    sd = model.state_dict()
    assert sorted(sd.keys()) == list(g[f"{tag}__keys"]), "state-dict keys differ from the reference's OBBModel"
    assert [repr(tuple(sd[k].shape)) for k in sorted(sd)] == list(g[f"{tag}__shapes"])
    assert sum(p.numel() for p in model.parameters()) == m["params"]
    with pytest.raises(NotImplementedError):
        model.init_criterion()


def test_head_keys_and_constructor(g):
    M.OBB.legacy = True
    head = M.OBB(nc=10, ne=1, ch=(32, 64))
    assert sorted(head.state_dict().keys()) == list(g["head_keys"])
    assert tuple(head.cv4[0][2].weight.shape) == (1, 8, 1, 1) and tuple(head.cv4[1][2].bias.shape) == (1,) and head.ne == 1


def test_guess_model_task():
    assert guess_model_task(YOLO("yolov8n-obb.yaml").model) == "obb"
    assert guess_model_task(dict(load_yaml("yolov8-obb.yaml", "n", 10))) == "obb" and guess_model_task(dict(load_yaml("yolov8-p2-repvgg-obb.yaml", "s", 3))) == "obb"
    assert guess_model_task("weights/yolov8s-p2-repvgg-obb.pt") == "obb" and guess_model_task("yolov8n-obb.yaml") == "obb"
    assert guess_model_task("yolov8n.yaml") == "detect" and guess_model_task("yolov8n-seg.yaml") == "segment"
    assert guess_model_task(dict(load_yaml("yolov8.yaml", "n", 10))) == "detect" and guess_model_task(dict(load_yaml("yolov8-seg.yaml", "n", 10))) == "segment"
    assert guess_model_task(DetectionModel(dict(load_yaml("yolov8.yaml", "n", 10)), nc=10, verbose=False)) == "detect"


@pytest.mark.parametrize("name", ["yolov8n.yaml", "yolov8n-seg.yaml"])
def test_task_obb_on_another_head_is_refused(name):
    with pytest.raises(ValueError, match="obb"):
        YOLO(name, task="obb")
    with pytest.raises(ValueError):
        YOLO("yolov8n-obb.yaml", task="detect")


@pytest.mark.parametrize("call,word", [
    (lambda y, x: y.train(data="synthetic:4"), "train"), (lambda y, x: y.val(data="synthetic:4"), "val"), (lambda y, x: y.track(x), "track"),
    (lambda y, x: y.predict(x, tile=64), "tile"), (lambda y, x: y.predict(x, augment=True), "augment")])
def test_unsupported_calls_raise_before_any_device_use(call, word):
    y = YOLO("yolov8n-obb.yaml")
    with pytest.raises(NotImplementedError, match=word):
        call(y, torch.zeros(1, 3, 64, 64))
    assert y.predictor is None and y.trainer is None and all(p.device.type == "cpu" for p in y.model.parameters())


# ---- host helpers against the recorded reference arrays -----------------------------------------------------------------------------
def test_regularize_rboxes_and_corners(g):
    boxes = torch.from_numpy(g["help_boxes"])
    t = boxes[:8, 4].numpy()
    hp = np.float32(np.pi / 2)
    assert t[0] == np.float32(-np.pi / 4) and t[1] == 0 and t[2] == np.nextafter(hp, np.float32(0)) and t[3] == hp and t[4] == np.float32(3 * np.pi / 4)
    reg = ops.regularize_rboxes(boxes)
    assert np.array_equal(reg.numpy(), g["help_regularized"])
    swapped = reg[:8, 2] != boxes[:8, 2]
    assert swapped.tolist() == [True, False, False, True, True, True, False, True]  # -pi/4 mod pi = 3pi/4: swap; pi/2 - ulp: none; pi/2: swap ...
    assert float(reg[:, 4].min()) >= 0 and float(reg[:, 4].max()) < float(hp) + 1e-6
    assert np.array_equal(ops.xywhr2xyxyxyxy(reg).numpy(), g["help_corners"])
    assert np.allclose(ops.xywhr2xyxyxyxy(reg.numpy()), g["help_corners"], rtol=0, atol=1e-4)  # the array form (numpy's own sin / cos)


def test_batch_probiou(g):
    boxes = torch.from_numpy(g["help_boxes"])
    got = metrics.batch_probiou(boxes[:12], boxes[8:])
    assert tuple(got.shape) == (12, 24) and np.array_equal(got.numpy(), g["help_probiou"])
    assert np.array_equal(metrics.batch_probiou(boxes[:12].numpy(), boxes[8:].numpy()).numpy(), g["help_probiou"])
    i64 = U.probiou64(boxes.numpy())  # the float64 form the fixtures' margins are computed with agrees with it
    assert np.abs(metrics.batch_probiou(boxes, boxes).numpy() - i64).max() < 1e-4


def test_results_obb(g):
    data = torch.from_numpy(g["help_obb_data"])
    hw = tuple(int(v) for v in g["help_orig_shape"])
    r = Results(np.zeros((*hw, 3), np.uint8), "x.jpg", {0: "a", 1: "b", 2: "c"}, obb=data)
    assert r.boxes is None and r.masks is None and isinstance(r.obb, OBB) and len(r) == len(data) and r.orig_shape == hw
    o = r.obb
    assert tuple(o.data.shape) == (len(data), 7) and torch.equal(o.xywhr, data[:, :5]) and torch.equal(o.conf, data[:, 5]) and torch.equal(o.cls, data[:, 6]) and o.id is None
    assert np.array_equal(o.xyxyxyxy.numpy(), g["help_xyxyxyxy"]) and tuple(o.xyxyxyxy.shape) == (len(data), 4, 2)
    assert np.array_equal(o.xyxyxyxyn.numpy(), g["help_xyxyxyxyn"]) and np.array_equal(o.xyxy.numpy(), g["help_xyxy"])
    assert len(r[2:5]) == 3 and torch.equal(r[2:5].obb.data, data[2:5]) and len(o[0]) == 1
    n = r.numpy()
    assert isinstance(n.obb.data, np.ndarray) and np.allclose(n.obb.xyxy, g["help_xyxy"], atol=1e-4) and n.obb.xyxyxyxyn.shape == (len(data), 4, 2)
    assert torch.equal(r.cpu().obb.data, data) and r.to(torch.float64).obb.data.dtype == torch.float64
    assert r.verbose().startswith("11 as, ")
    with pytest.raises(AssertionError):
        OBB(torch.zeros(2, 6), hw)


# ---- what the builder guarantees, re-asserted from the stored inputs -----------------------------------------------------------------
@pytest.mark.parametrize("name", list(U.NMS_CASES))
def test_nms_fixtures_are_decided_with_a_margin(g, name):
    counts, anchors, _, kw, _ = U.NMS_CASES[name]
    pred, theta = U.nms_inputs(name, int(g[f"nms_{name}__seed"]))
    M_, near, near_s = (float(v) for v in g[f"nms_{name}__margin"])
    assert tuple(pred.shape) == (len(counts), 4 + U.NC, anchors) and near > M_ >= 0 and near_s > M_
    assert float((pred[:, 4:] - U.CONF).abs().min()) > M_
    kept = [int(k) for k in g[f"nms_{name}__n"]]
    idx = np.split(g[f"nms_{name}__idx"], np.cumsum(kept)[:-1])
    for b in range(len(counts)):
        cand, boxes, _ = U.sorted_candidates(pred, theta, b, kw)
        if len(boxes) < 2:
            continue
        i64 = U.probiou64(boxes.numpy())
        up = np.triu(np.ones_like(i64, bool), 1)
        assert not np.isnan(i64[up]).any() and np.abs(i64[up] - U.IOU).min() > M_, "a pair within M of the threshold"
        keep = U.fast_nms(i64, U.IOU)[: kw.get("max_det", 300)]  # the float64 decision IS the reference's
        assert np.array_equal(cand[keep].numpy(), idx[b])


def test_chain_fixture_tells_fast_from_greedy(g):
    pred, theta = U.nms_inputs("chain", int(g["nms_chain__seed"]))
    cand, boxes, _ = U.sorted_candidates(pred, theta, 0, {})
    i64 = U.probiou64(boxes.numpy())
    assert i64[0, 1] >= U.IOU and i64[1, 2] >= U.IOU and i64[0, 2] < U.IOU  # A suppresses B, B alone overlaps C
    assert U.greedy_nms(i64, U.IOU) == [0, 2] and U.fast_nms(i64, U.IOU) == [0]
    assert g["nms_chain__idx"].tolist() == [int(cand[0])], "the reference drops C, which a greedy scan keeps"


def test_case_inputs_are_as_intended(g):
    for name, (counts, anchors, _, kw, _) in U.NMS_CASES.items():
        pred, theta = U.nms_inputs(name, int(g[f"nms_{name}__seed"]))
        if name not in ("few", "chain"):
            assert U.candidate_counts(pred, {}) == counts
    pred, theta = U.nms_inputs("few", int(g["nms_few__seed"]))
    assert U.candidate_counts(pred, {}) == [0, 1, 2] and torch.equal(pred[2, :, 9], pred[2, :, 41]) and theta[2, 9] == theta[2, 41]
    assert U.candidate_counts(U.nms_inputs("lds_cap", int(g["nms_lds_cap__seed"]))[0], {})[0] > U.LDS_CAP > 300
    assert int(g["nms_crowd__n"][0]) == U.NMS_CASES["crowd"][3]["max_det"] < 400
    assert U.candidate_counts(U.nms_inputs("max_nms", 1)[0], {})[0] > U.NMS_CASES["max_nms"][3]["max_nms"]
    pred, _ = U.nms_inputs("degenerate", int(g["nms_degenerate__seed"]))
    best = pred[0, 4:].amax(0) > U.CONF
    assert int((pred[0, 2][best] == 0).sum()) == 6 and int((pred[0, 3][best] == 0).sum()) == 6
    assert int(g["nms_same_place__n"][0]) > int(g["nms_same_place_agnostic__n"][0])


# ---- the C interface without a device ------------------------------------------------------------------------------------------------
def test_entry_points_validate_without_gpu(tmp_path):
    import ctypes
    import os
    import subprocess

    from drone_yolo_amd import _lib as L
    from tests._util import ROOT

    h = L.lib()
    assert h.dy_obb_decode(ctypes.byref(L.ObbDecodeDesc()), None) == -1 and b"dy_obb_decode" in h.dy_last_error_string()
    assert h.dy_nms_rotated(ctypes.byref(L.NmsDesc()), None, None) == -1 and h.dy_scale_rboxes(None, None, None, 1, 1, None) == -1
    buf = ctypes.cast((ctypes.c_float * 64)(), ctypes.c_void_p)
    d = L.NmsDesc()
    d.pred = d.out = d.out_count = d.workspace = buf
    d.batch, d.nc, d.anchors, d.conf_thres, d.iou_thres, d.max_det, d.max_nms, d.workspace_bytes = 1, 3, 100, 0.25, 0.45, 300, 30000, h.dy_nms_workspace_bytes(1, 100)
    assert h.dy_nms_rotated(ctypes.byref(d), buf, None) == -4 and b"dy_nms_rotated: workspace" in h.dy_last_error_string()  # DY_ERR_WORKSPACE: the table lies behind a dy_nms workspace
    d.multi_label = 1
    assert h.dy_nms_rotated(ctypes.byref(d), buf, None) == -2  # DY_ERR_UNSUPPORTED
    assert h.dy_nms(ctypes.byref(L.NmsDesc()), None) == -1 and b"dy_nms: null" in h.dy_last_error_string()  # the shared checks still name their caller
    assert h.dy_nms_rotated_workspace_bytes(2, 34000) == h.dy_nms_workspace_bytes(2, 34000) + 2 * 5 * 34000 * 4 and h.dy_nms_rotated_workspace_bytes(0, 5) == -1
    assert h.dy_nms_rotated_lds_cap() == U.LDS_CAP
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include "dyolo.h"\nint main(){printf("%zu\\n", sizeof(dy_obb_decode_desc));return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "s")])
    assert int(subprocess.check_output([str(tmp_path / "s")])) == ctypes.sizeof(L.ObbDecodeDesc)
