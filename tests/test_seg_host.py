"""CPU: the segmentation surface without a device — model building against the reference's key lists (tests/golden/seg.npz,
tools/make_seg_golden.py), task plumbing, save / load, the refusals, the C-ABI checks of the three new entry points, ``Masks``, and the
weight repack of Proto's transposed convolution."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from drone_yolo_amd import YOLO
from drone_yolo_amd import hip_ops as H
from drone_yolo_amd.engine.results import Masks, Results
from drone_yolo_amd.nn import modules as M
from drone_yolo_amd.nn.tasks import DetectionModel, SegmentationModel, guess_model_task, parse_model, yaml_model_load
from oracle import drone_yolo_oracle as O
from tests._util import ROOT, golden, meta


@pytest.fixture(scope="module")
def g():
    return golden("seg.npz")


@pytest.mark.parametrize("tag,yaml_name", [("segn96", "yolov8n-p2-repvgg-seg.yaml"), ("seg3n64x96", "yolov8n-seg.yaml")])
def test_parse_model_builds_the_reference_graph(g, tag, yaml_name):
    m = meta(g, tag)
    d = yaml_model_load(yaml_name)
    d["nc"] = m["nc"]
    layers, save = parse_model(dict(d), ch=3, verbose=False)
    assert isinstance(layers[-1], M.Segment) and isinstance(layers[-1].proto, M.Proto) and isinstance(layers[-1].proto.upsample, torch.nn.ConvTranspose2d)
    model = SegmentationModel(dict(d), nc=m["nc"], verbose=False)
    sd = model.state_dict()
    assert sorted(sd.keys()) == [str(k) for k in g[f"{tag}__keys"]]
    assert [repr(tuple(sd[k].shape)) for k in sorted(sd.keys())] == [str(s) for s in g[f"{tag}__shapes"]]
    assert sum(p.numel() for p in model.parameters()) == m["params"]
    head = model.model[-1]
    assert head.nm == 32 and head.npr == 64 and head.nl == (4 if "p2" in yaml_name else 3)  # npr 256 scaled by the width multiple 0.25
    assert list(head.stride) == ([4, 8, 16, 32] if "p2" in yaml_name else [8, 16, 32])


def test_segment_head_keys_match_the_reference(g):
    M.Segment.legacy = True
    head = M.Segment(nc=10, nm=32, npr=64, ch=(32, 64))
    assert sorted(head.state_dict().keys()) == [str(k) for k in g["seghead_keys"]]


def test_task_is_taken_from_the_head_or_the_name():
    assert YOLO("yolov8n-p2-repvgg-seg.yaml").task == "segment"
    y = YOLO("yolov8n-seg.yaml")
    assert y.task == "segment" and isinstance(y.model, SegmentationModel) and set(y.task_map) == {"detect", "segment"}
    det = YOLO("yolov8n-p2-repvgg.yaml")
    assert det.task == "detect" and type(det.model) is DetectionModel
    assert guess_model_task("runs/yolov8s-seg.pt") == "segment" and guess_model_task("yolov8s.pt") == "detect"
    assert guess_model_task(y.model) == "segment" and guess_model_task(det.model) == "detect" and guess_model_task(y.model.yaml) == "segment"
    with pytest.raises(ValueError):
        YOLO("yolov8n-seg.yaml", task="detect")
    with pytest.raises(NotImplementedError):
        YOLO("yolov8n-seg.yaml", task="pose")


def test_save_load_round_trips_weights_and_task(tmp_path):
    y = YOLO("yolov8n-seg.yaml")
    sd = O.seeded_state_dict(y.model.state_dict(), 7)
    y.model.load_state_dict(sd)
    y.save(tmp_path / "seg.pt")
    z = YOLO(str(tmp_path / "seg.pt"))
    assert z.task == "segment" and isinstance(z.model, SegmentationModel) and isinstance(z.model.model[-1], M.Segment)
    got = z.model.state_dict()
    assert sorted(got) == sorted(sd)
    for k, v in sd.items():  # (the checkpoint holds the module graph in float16, as the reference's does)
        assert torch.equal(got[k].float(), v.half().float() if v.is_floating_point() else v), k


def test_unsupported_combinations_raise_before_any_device_use():
    y = YOLO("yolov8n-seg.yaml")
    x = torch.zeros(1, 3, 64, 64)
    for kw, word in ((dict(tile=64), "tile"), (dict(augment=True), "augment"), (dict(mode="track"), "track")):
        with pytest.raises(NotImplementedError, match=word):
            y.predict(x, **kw)
        assert y.predictor is None
    with pytest.raises(NotImplementedError, match="track"):
        y.track(x)
    with pytest.raises(NotImplementedError, match="train"):
        y.train(data="synthetic:4", epochs=1)
    with pytest.raises(NotImplementedError, match="val"):
        y.val(data="synthetic:4")
    with pytest.raises(NotImplementedError, match="train"):
        y.model.init_criterion()
    assert y.predictor is None and y.trainer is None


def test_new_entry_points_validate_without_gpu():
    import drone_yolo_amd._lib as L

    h = L.lib()
    buf = (ctypes.c_float * 256)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert h.dy_process_mask(None, None) == -1 and h.dy_mask_gather(None, None) == -1
    assert h.dy_process_mask(ctypes.byref(L.ProcessMaskDesc()), None) == -1 and b"null" in h.dy_last_error_string()
    assert h.dy_mask_gather(ctypes.byref(L.MaskGatherDesc()), None) == -1 and b"null" in h.dy_last_error_string()
    assert h.dy_depth_to_space2_nhwc(None, None, 1, 4, 4, 8, 32, 8, L.DY_F16, None) == -1
    d = L.ProcessMaskDesc()
    d.protos = d.side = d.counts = d.offsets = d.window = d.out = p
    d.batch, d.max_det, d.nm, d.mh, d.mw, d.ld_p, d.oh, d.ow, d.total = 1, 8, 16, 4, 4, 16, 16, 16, 1
    assert h.dy_process_mask(ctypes.byref(d), None) == -2 and b"nm = 32" in h.dy_last_error_string()
    d.nm, d.ld_p, d.total = 32, 32, 0
    assert h.dy_process_mask(ctypes.byref(d), None) == 0  # no detections: returns without a launch
    d.total = 9
    assert h.dy_process_mask(ctypes.byref(d), None) == -1  # more masks than batch * max_det rows
    m = L.MaskGatherDesc()
    m.rows = m.counts = m.index = m.out = m.pred = p
    m.batch, m.max_det, m.nm, m.anchors, m.pred_ch, m.pred_c0 = 1, 8, 16, 100, 30, 14
    assert h.dy_mask_gather(ctypes.byref(m), None) == -2
    m.nm = 32
    assert h.dy_mask_gather(ctypes.byref(m), None) == -1 and b"outside pred" in h.dy_last_error_string()  # 14 + 32 > 30 channels
    assert h.dy_depth_to_space2_nhwc(p, p, 1, 4, 4, 12, 48, 12, L.DY_F32, None) == -2  # c % 8 != 0
    assert h.dy_depth_to_space2_nhwc(p, p, 1, 4, 4, 8, 32, 8, L.DY_FP8, None) == -1
    assert h.dy_depth_to_space2_nhwc(p, p, 1, 4, 4, 8, 24, 8, L.DY_F16, None) == -1  # source pitch below 4c
    # process_mask(out=): every clause of the refusal, each tensor with exactly one defect (CPU tensors: the device clause comes last, so
    # the others are reached here; a correct tensor that is merely on the CPU is refused by that last clause)
    protos, side, count = torch.zeros(1, 32, 4, 4), torch.zeros(1, 8, 36), torch.zeros(1, dtype=torch.int32)
    n_out = 2 * 6 * 5
    base = torch.zeros(n_out + 16, dtype=torch.uint8)
    lead = (-base.data_ptr()) % 8  # base[lead:] is 8-byte aligned
    aligned, off4 = base[lead : lead + n_out], base[lead + 4 : lead + 4 + n_out]
    assert aligned.data_ptr() % 8 == 0 and off4.data_ptr() % 8 == 4 and aligned.is_contiguous() and off4.is_contiguous()
    strided = torch.zeros(2 * n_out + 16, dtype=torch.uint8)
    strided = strided[(-strided.data_ptr()) % 8 :][: 2 * n_out : 2]
    assert strided.numel() == n_out and strided.data_ptr() % 8 == 0 and not strided.is_contiguous()
    for bad, word in ((aligned.view(torch.int8), "dtype"), (aligned[:-1], "elements"), (base[lead : lead + n_out + 8], "elements"),
                      (strided, "contiguous"), (off4, "aligned"), (aligned, "device")):
        with pytest.raises(ValueError, match=f"out must be .*: .*{word}"):
            H.process_mask(protos, side, count, [2], (6, 5), out=bad)


def test_new_struct_layouts_match_the_header(tmp_path):
    import subprocess

    import drone_yolo_amd._lib as L

    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include "dyolo.h"\nint main(){printf("%zu %zu\\n", sizeof(dy_mask_gather_desc), sizeof(dy_process_mask_desc));return 0;}\n')
    exe = tmp_path / "s"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert sizes == [ctypes.sizeof(L.MaskGatherDesc), ctypes.sizeof(L.ProcessMaskDesc)]


def test_masks_container():
    data = (torch.arange(3 * 4 * 5).view(3, 4, 5) % 2).to(torch.uint8)
    m = Masks(data, (8, 10))
    assert m.shape == (3, 4, 5) and m.orig_shape == (8, 10) and len(m) == 3
    assert m[1].shape == (1, 4, 5) and torch.equal(m[1].data[0], data[1]) and m[[0, 2]].shape == (2, 4, 5)
    assert isinstance(m.cpu().data, torch.Tensor) and isinstance(m.numpy().data, np.ndarray) and m.numpy().data.dtype == np.uint8
    assert m.to("cpu").data.dtype == torch.uint8
    for attr in ("xy", "xyn"):
        with pytest.raises(NotImplementedError, match="findContours"):
            getattr(m, attr)
    rows = torch.tensor([[0, 0, 4, 4, 0.9, 1], [1, 1, 5, 3, 0.8, 0], [2, 0, 5, 4, 0.7, 1]], dtype=torch.float32)
    r = Results(torch.zeros(3, 4, 5), "a.jpg", {0: "a", 1: "b"}, boxes=rows, masks=data)
    assert r.masks.shape == (3, 4, 5) and r[1].masks.shape == (1, 4, 5) and len(r[1]) == 1
    assert isinstance(r.numpy().masks.data, np.ndarray) and isinstance(r.cpu().masks.data, torch.Tensor) and r.to("cpu").masks is not None
    assert len(r.summary()) == 3 and set(r.summary()[0]) == {"name", "class", "confidence", "box"} and r.verbose() == "1 a, 2 bs, "
    assert Results(torch.zeros(3, 4, 5), "a.jpg", {0: "a"}, boxes=rows[:0]).masks is None


def test_deconv_repack_equals_conv_transpose2d():
    g_ = torch.Generator().manual_seed(5)
    w, b, x = torch.randn(12, 16, 2, 2, generator=g_), torch.randn(16, generator=g_), torch.randn(2, 12, 5, 7, generator=g_)
    ref = F.conv_transpose2d(x, w, b, stride=2)
    w1, b4 = H.deconv2x2_as_conv1x1(w, b)
    assert tuple(w1.shape) == (64, 12, 1, 1) and tuple(b4.shape) == (64,)
    y = F.conv2d(x, w1, b4)  # (2, 4 * 16, 5, 7), channel (a * 2 + b) * 16 + o
    got = y.view(2, 2, 2, 16, 5, 7).permute(0, 3, 4, 1, 5, 2).reshape(2, 16, 10, 14)  # the depth-to-space of dy_depth_to_space2_nhwc
    assert torch.allclose(got, ref, rtol=1e-5, atol=1e-5)
    w0, b0 = H.deconv2x2_as_conv1x1(w, None)
    assert torch.equal(w0, w1) and not b0.any()
    with pytest.raises(ValueError):
        H.deconv2x2_as_conv1x1(torch.zeros(4, 4, 3, 3), None)
