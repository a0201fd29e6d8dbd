"""CPU: the pose task's construction, refusals, host helpers, crop arithmetic and fixtures (tests/golden/pose.npz, tools/make_pose_golden.py)."""
import numpy as np
import pytest
import torch

from drone_yolo_amd import YOLO
from drone_yolo_amd.engine import crops as CR
from drone_yolo_amd.engine.results import Keypoints, Results
from drone_yolo_amd.nn import modules as M
from drone_yolo_amd.nn.tasks import DetectionModel, PoseModel, guess_model_task
from drone_yolo_amd.utils import ops
from oracle import letterbox_oracle as LB
from tests import _pose_util as U
from tests._util import golden, load_yaml, meta


@pytest.fixture(scope="module")
def g():
    return golden("pose.npz")


# ---- construction and task ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tag", [("yolov8n-pose.yaml", "pose3n64x96"), ("yolov8n-p2-repvgg-pose.yaml", "posen64x96")])
def test_yolo_builds_a_pose_model_with_the_reference_state_dict(g, name, tag):
    y = YOLO(name)
    assert y.task == "pose" and type(y.model) is PoseModel and isinstance(y.model.model[-1], M.Pose) and y.overrides["task"] == "pose"
    assert y.model.kpt_shape == (17, 3) and y.model.yaml["nc"] == 1
    m = meta(g, tag)
    d = dict(load_yaml(m["yaml"], m["scale"], m["nc"]))
    assert tuple(d["kpt_shape"]) == m["kpt_shape"]
    model = PoseModel(d, nc=m["nc"], verbose=False)
    sd = model.state_dict()
    assert sorted(sd.keys()) == list(g[f"{tag}__keys"]), "state-dict keys differ from the reference's PoseModel"
    assert [repr(tuple(sd[k].shape)) for k in sorted(sd)] == list(g[f"{tag}__shapes"])
    assert sum(p.numel() for p in model.parameters()) == m["params"]
    with pytest.raises(NotImplementedError):
        model.init_criterion()


def test_kpt_shape_comes_from_the_yaml_or_the_data():
    d = dict(load_yaml("yolov8-pose.yaml", "n", 1))
    d["kpt_shape"] = [4, 2]
    model = PoseModel(d, verbose=False)
    assert model.kpt_shape == (4, 2) and model.model[-1].nk == 8 and tuple(model.model[-1].cv4[0][2].weight.shape) == (8, 16, 1, 1)
    model = PoseModel(dict(load_yaml("yolov8-pose.yaml", "n", 1)), data_kpt_shape=(5, 3), verbose=False)
    assert model.kpt_shape == (5, 3) and model.model[-1].nk == 15


@pytest.mark.parametrize("name", ["a", "b"])
def test_head_keys_and_constructor(g, name):
    spec = U.HEADS[name]
    M.Pose.legacy = True
    head = M.Pose(nc=spec["nc"], kpt_shape=spec["kpt_shape"], ch=U.HEAD_CH)
    nk = spec["kpt_shape"][0] * spec["kpt_shape"][1]
    c4 = max(U.HEAD_CH[0] // 4, nk)
    assert sorted(head.state_dict().keys()) == list(g[f"head_{name}_keys"])
    assert head.nk == nk and tuple(head.kpt_shape) == spec["kpt_shape"]
    assert tuple(head.cv4[0][0].conv.weight.shape) == (c4, 32, 3, 3) and tuple(head.cv4[1][1].conv.weight.shape) == (c4, c4, 3, 3)
    assert tuple(head.cv4[1][2].weight.shape) == (nk, c4, 1, 1) and tuple(head.cv4[1][2].bias.shape) == (nk,)


def test_served_width_pads_the_51_channel_branch_only_in_the_packs():
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        assert M.Pose.served_width(51, dt) == 64 and M.Pose.served_width(64, dt) == 64 and M.Pose.served_width(8, dt) == 8 and M.Pose.served_width(128, dt) == 128
        assert M.Pose.served_width(51, dt) % 8 == 0


def test_guess_model_task():
    assert guess_model_task(YOLO("yolov8n-pose.yaml").model) == "pose"
    assert guess_model_task(dict(load_yaml("yolov8-pose.yaml", "n", 1))) == "pose" and guess_model_task(dict(load_yaml("yolov8-p2-repvgg-pose.yaml", "s", 1))) == "pose"
    assert guess_model_task("weights/yolov8s-p2-repvgg-pose.pt") == "pose" and guess_model_task("yolov8n-pose.yaml") == "pose"
    assert guess_model_task("yolov8n.yaml") == "detect" and guess_model_task("yolov8n-seg.yaml") == "segment" and guess_model_task("yolov8n-obb.yaml") == "obb"
    assert guess_model_task(DetectionModel(dict(load_yaml("yolov8.yaml", "n", 10)), nc=10, verbose=False)) == "detect"


@pytest.mark.parametrize("name", ["yolov8n.yaml", "yolov8n-seg.yaml", "yolov8n-obb.yaml"])
def test_task_pose_on_another_head_is_refused(name):
    with pytest.raises(ValueError, match="pose"):
        YOLO(name, task="pose")
    for task in ("detect", "segment", "obb"):
        with pytest.raises(ValueError):
            YOLO("yolov8n-pose.yaml", task=task)
    assert YOLO("yolov8n-pose.yaml", task="pose").task == "pose"


def test_checkpoint_round_trip_carries_the_task(tmp_path):
    y = YOLO("yolov8n-pose.yaml")
    y.save(tmp_path / "p.pt")
    again = YOLO(str(tmp_path / "p.pt"))
    assert again.task == "pose" and type(again.model) is PoseModel and again.model.kpt_shape == (17, 3)
    a, b = y.model.state_dict(), again.model.state_dict()
    assert sorted(a) == sorted(b) and all(torch.equal(a[k].half().float() if a[k].is_floating_point() else a[k], b[k]) for k in a)


_X = torch.zeros(1, 3, 64, 64)
_F = np.zeros((2, 90, 140, 3), np.uint8)


@pytest.mark.parametrize("call,word", [
    (lambda y: y.train(data="synthetic:4"), "train"), (lambda y: y.val(data="synthetic:4"), "val"), (lambda y: y.track(_X), "track"),
    (lambda y: y.track(list(_F)), "track"), (lambda y: y.predict(_X, tile=64), "tile"), (lambda y: y.predict(list(_F), tile=64), "tile"),
    (lambda y: y.predict(_X, augment=True), "augment")])
def test_unsupported_calls_raise_before_any_device_use(call, word):
    y = YOLO("yolov8n-pose.yaml")
    with pytest.raises(NotImplementedError, match=word):
        call(y)
    assert y.predictor is None and y.trainer is None and all(p.device.type == "cpu" for p in y.model.parameters())


@pytest.mark.parametrize("call,word", [
    (lambda y: y.predict(_F, crops=[np.array([[5.0, 5.0, 5.0, 9.0]]), np.zeros((0, 4))]), "empty"),
    (lambda y: y.predict([_F[0], np.zeros((80, 140, 3), np.uint8)], crops=[np.array([[5.0, 5.0, 9.0, 9.0]])] * 2), "one shape"),
    (lambda y: y.predict(_X, crops=[np.array([[5.0, 5.0, 9.0, 9.0]])]), "tensor"),
    (lambda y: y.predict(torch.zeros(2, 90, 140, 3, dtype=torch.uint8), crops=[np.array([[5.0, 5.0, 9.0, 9.0]])] * 2), "tensor"),
    (lambda y: y.predict(_F, crops=[np.array([[5.0, 5.0, 9.0, 9.0]])]), "per frame")])
def test_bad_crop_calls_raise_value_error_before_any_device_use(call, word):
    y = YOLO("yolov8n-pose.yaml")
    with pytest.raises(ValueError, match=word):
        call(y)
    assert y.predictor is None and all(p.device.type == "cpu" for p in y.model.parameters())


@pytest.mark.parametrize("name", ["yolov8n.yaml", "yolov8n-seg.yaml", "yolov8n-obb.yaml"])
def test_crops_on_another_task_raise_value_error(name):
    y = YOLO(name)
    with pytest.raises(ValueError, match="crops"):
        y.predict(_F, crops=[np.array([[5.0, 5.0, 9.0, 9.0]])] * 2)
    assert y.predictor is None


def test_head_refuses_training_mode_and_fp8_without_a_device():
    head = M.Pose(nc=1, kpt_shape=(4, 2), ch=(32, 64))
    head.train()
    with pytest.raises(NotImplementedError, match="training"):
        head([torch.zeros(1, 32, 4, 4), torch.zeros(1, 64, 2, 2)])
    head.eval()
    with pytest.raises(NotImplementedError, match="storage"):
        head([torch.zeros(1, 32, 4, 4).to(torch.float8_e4m3fn), torch.zeros(1, 64, 2, 2).to(torch.float8_e4m3fn)])


# ---- host helpers against the recorded reference arrays -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(U.SCALE_CASES))
def test_scale_coords_and_keypoints_against_the_reference(g, name):
    in_hw, orig_hw = U.SCALE_CASES[name]
    kp = U.scale_inputs(int(g[f"sc_{name}_seed"]), in_hw)
    scaled = ops.scale_coords(in_hw, kp.clone(), orig_hw)
    assert np.array_equal(scaled.numpy(), g[f"sc_{name}_scaled"])
    gain, px, py = ops.letterbox_params(in_hw, orig_hw)  # scale_boxes rounds the pad, scale_coords does not
    raw = ((in_hw[1] - orig_hw[1] * gain) / 2, (in_hw[0] - orig_hw[0] * gain) / 2)
    assert (px, py) != raw and (raw[0] != round(raw[0])) == (name == "pad_x") and (raw[1] != round(raw[1])) == (name == "pad_y")
    res = Keypoints(scaled.clone(), orig_hw)
    assert res.has_visible and np.array_equal(res.data.numpy(), g[f"sc_{name}_out"]) and np.array_equal(res.xy.numpy(), g[f"sc_{name}_xy"])
    assert np.array_equal(res.xyn.numpy(), g[f"sc_{name}_xyn"]) and np.array_equal(res.conf.numpy(), g[f"sc_{name}_conf"])
    hidden = kp[..., 2] < 0.5
    assert bool(hidden.any()) and bool((res.xy[hidden] == 0).all()) and bool((res.xy[~hidden] == scaled[..., :2][~hidden]).all())
    as_np = Keypoints(scaled.numpy().copy(), orig_hw)  # numpy rows take the same path
    assert np.array_equal(as_np.data, g[f"sc_{name}_out"]) and np.array_equal(as_np.xyn, g[f"sc_{name}_xyn"])
    xy_only = Keypoints(scaled[..., :2].clone(), orig_hw)
    assert not xy_only.has_visible and xy_only.conf is None and torch.equal(xy_only.xy, scaled[..., :2])
    assert np.array_equal(ops.clip_coords(kp.numpy()[..., :2].copy(), in_hw), ops.clip_coords(kp[..., :2].clone(), in_hw).numpy())


def test_results_carry_keypoints(g):
    rows, kp = g["posen64x96__det"][:4], g["posen64x96__kpts"][:4]
    r = Results(np.zeros((64, 96, 3), np.uint8), "x.jpg", {0: "person"}, boxes=torch.from_numpy(rows), keypoints=torch.from_numpy(kp))
    assert len(r) == 4 and isinstance(r.keypoints, Keypoints) and tuple(r.keypoints.data.shape) == (4, 17, 3) and r.crop is None
    assert len(Results(np.zeros((64, 96, 3), np.uint8), "x.jpg", {0: "person"}, keypoints=torch.from_numpy(kp))) == 4
    r.crop = (0, 1, 2, 30, 40)
    for other in (r.cpu(), r.numpy(), r.to("cpu"), r[1:3]):
        assert other.keypoints is not None and other.crop == r.crop and len(other.keypoints) == len(other.boxes)
    assert np.array_equal(r[1:3].keypoints.data.numpy(), kp[1:3]) and isinstance(r.numpy().keypoints.data, np.ndarray)
    assert Results(np.zeros((64, 96, 3), np.uint8), "x.jpg", {0: "person"}, boxes=torch.from_numpy(rows)).keypoints is None


# ---- crop rectangles and the slicer's table -------------------------------------------------------------------------------------------
def test_crop_rectangles_and_letterbox_table_against_the_oracle_geometry():
    frames = list(U.crop_frames())
    rects = CR.crop_rects(frames, U.CROP_BOXES, U.CROP_EXPAND)
    assert rects == U.CROP_RECTS
    H_, W_ = U.CROP_FRAMES_HW
    flat = [(f, b) for f, bx in enumerate(U.CROP_BOXES) for b in bx]
    for (f, b), rect in zip(flat, rects):  # the pipeline's arithmetic, in Python floats
        x1, y1, x2, y2 = (float(v) for v in b)
        w, h = x2 - x1, y2 - y1
        assert rect == (f, int(max(0, x1 - w * 0.2)), int(max(0, y1 - h * 0.2)), int(min(W_, x2 + w * 0.2)), int(min(H_, y2 + h * 0.2)))
    sizes = [(r[3] - r[1], r[4] - r[2]) for r in rects]
    assert rects[0][1:3] == (0, 0) and rects[1][3:] == (W_, H_) and sizes[2][0] == 64 and sizes[3][1] > 4 * sizes[3][0] and sizes[4] == (9, 7)
    for imgsz in (64, 66):
        table = CR.crop_table(rects, imgsz)
        assert table.dtype == np.int32 and table.shape == (5, CR.CROP_COLS)
        for row, (f, x0, y0, x1, y1) in zip(table.tolist(), rects):
            nw, nh, top, bottom, left, right = LB.letterbox_geometry((y1 - y0, x1 - x0), (imgsz, imgsz), auto=False)
            assert row == [f, x0, y0, x1 - x0, y1 - y0, nw, nh, top, left]
            assert nh + top + bottom == imgsz and nw + left + right == imgsz
            crop = frames[f][y0:y1, x0:x1]
            assert LB.letterbox(crop, (imgsz, imgsz), auto=False).shape[:2] == (imgsz, imgsz)
    t64 = CR.crop_table(rects, 64).tolist()
    assert t64[2][5:7] == [64, 42] == t64[2][3:5], "the 64-wide crop is copied at imgsz 64"
    assert t64[4][5] > t64[4][3], "the 9 x 7 crop is upscaled"


def test_crop_rects_take_lists_and_float32_boxes():
    frames = list(U.crop_frames())
    as_lists = [b.tolist() for b in U.CROP_BOXES]
    as_f32 = [b.astype(np.float32) for b in U.CROP_BOXES]
    assert CR.crop_rects(frames, as_lists, 0.2) == U.CROP_RECTS
    f32 = CR.crop_rects(frames, as_f32, 0.2)
    assert [r[0] for r in f32] == [r[0] for r in U.CROP_RECTS] and len(f32) == 5
    assert CR.crop_rects(frames, [U.CROP_BOXES[0], np.zeros((0, 4))], 0.2) == U.CROP_RECTS[:3]
    with pytest.raises(ValueError, match="no boxes"):
        CR.crop_rects(frames, [np.zeros((0, 4)), []], 0.2)
