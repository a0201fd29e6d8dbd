"""CPU: the host side of the device augmentation (data/augment.py, the new training arguments, the dataset-YAML loader, the C-ABI checks
of dy_augment_u8_nchw).  tests/golden/train_aug.npz holds what the REAL reference computed (tools/make_aug_golden.py): Mosaic._mosaic4's
canvases and labels, RandomPerspective.__call__'s matrices, labels and kept-box masks, RandomFlip's labels."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from drone_yolo_amd.data import augment as A
from tests._util import ROOT, golden

G = golden("train_aug.npz")
S = int(G["S"])


def _shape(i):
    return tuple(int(v) for v in G[f"img_{i}"].shape[:2])


def _paste(ids, yc, xc):
    """The 2S x 2S canvas rebuilt from ``mosaic_placement``'s rectangles (HWC, 114 elsewhere)."""
    a, b, pads = A.mosaic_placement(S, yc, xc, [_shape(i) for i in ids])
    canvas = np.full((2 * S, 2 * S, 3), 114, dtype=np.uint8)
    for i, ra, rb in zip(ids, a, b):
        canvas[ra[1] : ra[3], ra[0] : ra[2]] = G[f"img_{i}"][rb[1] : rb[3], rb[0] : rb[2]]
    return canvas, a, b, pads


def test_mosaic_placement_and_labels_match_the_reference():
    for k in range(int(G["n_mosaic"])):
        yc, xc = (int(v) for v in G[f"mos{k}_center"])
        ids = [int(v) for v in G[f"mos{k}_ids"]]
        canvas, a, b, pads = _paste(ids, yc, xc)
        assert np.array_equal(canvas, G[f"mos{k}_canvas"]), f"mosaic {k}: the rectangles do not rebuild the reference's canvas"
        assert np.array_equal(np.array(pads), G[f"mos{k}_pads"]), f"mosaic {k}: (padw, padh)"
        for ra, rb in zip(a, b):  # the two rectangles of an image have one size
            assert (ra[2] - ra[0], ra[3] - ra[1]) == (rb[2] - rb[0], rb[3] - rb[1])
        src = [(G[f"lab_{i}"][:, :1], G[f"lab_{i}"][:, 1:], _shape(i), pads[j]) for j, i in enumerate(ids)]
        cls, boxes = A.place_labels(src, (2 * S, 2 * S))
        assert boxes.dtype == np.float32 and np.array_equal(cls, G[f"mos{k}_cls"])
        assert np.array_equal(boxes, G[f"mos{k}_boxes"]), f"mosaic {k}: concatenated labels differ from the reference's"


def test_affine_matrix_and_warped_labels_match_the_reference():
    n = 0
    for name in (str(v) for v in G["persp_names"]):
        for tag in ("m", "p"):
            key = f"persp_{tag}_{name}"
            if f"{key}_M" not in G.files:
                continue
            n += 1
            px, py, ang, sc, shx, shy, tx, ty = (float(v) for v in G[f"{key}_draws"])
            canvas = (2 * S, 2 * S) if tag == "m" else (S, S)
            m = A.affine_matrix(canvas, (S, S), ang, sc, shx, shy, px, py, tx, ty)
            assert m.dtype == np.float32 and np.array_equal(m, G[f"{key}_M"]), f"{key}: M"
            if tag == "m":
                cls, boxes = G["mos0_cls"], G["mos0_boxes"].copy()
            else:
                cls, boxes = A.place_labels([(G["lab_3"][:, :1], G["lab_3"][:, 1:], (S, S), (0, 0))], (S, S), cat=False)
            new, keep = A.warp_labels(boxes, m, sc, (S, S), perspective=bool(px))
            assert np.array_equal(keep, G[f"{key}_keep"]), f"{key}: kept-box mask"
            assert np.array_equal(new, G[f"{key}_new"]), f"{key}: warped and clipped boxes"
            assert np.array_equal(new[keep], G[f"{key}_out_boxes"]) and np.array_equal(cls[keep], G[f"{key}_out_cls"])
    assert n >= 8
    # the matrices the exact GPU case rests on are pure integer translations
    assert np.array_equal(G["persp_m_shift_17_40_M"], np.array([[1, 0, -17], [0, 1, -40], [0, 0, 1]], dtype=np.float32))
    assert np.array_equal(A.inverse_matrix(G["persp_m_shift_17_40_M"]), np.array([1, 0, 17, 0, 1, 40, 0, 0, 1], dtype=np.float32))


def test_flips_and_normalisation_match_the_reference():
    for tag, ud, lr in (("none", False, False), ("ud", True, False), ("lr", False, True), ("both", True, True)):
        got = A.flip_and_normalise(G["flip_in"].copy(), (S, S), ud, lr)
        assert got.dtype == np.float32 and np.array_equal(got, G[f"flip_{tag}"]), tag


def test_transform_labels_composes_the_reference_path():
    """One mosaic sample end to end equals the three recorded reference stages chained (mosaic 0 -> the 17/40 shift -> flips)."""
    ids = [int(v) for v in G["mos0_ids"]]
    yc, xc = (int(v) for v in G["mos0_center"])
    _, _, pads = A.mosaic_placement(S, yc, xc, [_shape(i) for i in ids])
    src = [(G[f"lab_{i}"][:, :1], G[f"lab_{i}"][:, 1:], _shape(i), pads[j]) for j, i in enumerate(ids)]
    m = G["persp_m_shift_centre_M"]
    cls, boxes = A.transform_labels(src, (2 * S, 2 * S), m, 1.0, (S, S), perspective=False, flipud=True, fliplr=True)
    assert np.array_equal(boxes, G["flip_both"]) and np.array_equal(cls, G["persp_m_shift_centre_out_cls"])
    assert boxes.min() >= 0.0 and boxes.max() <= 1.0


def test_training_arguments():
    from drone_yolo_amd.engine.trainer import get_cfg

    cfg = get_cfg(dict(mosaic=0.5, device_augment=True))  # (KeyError before the feature)
    assert cfg["mosaic"] == 0.5 and cfg["device_augment"] is True
    ref = dict(mosaic=1.0, close_mosaic=10, degrees=0.0, translate=0.1, scale=0.5, shear=0.0, perspective=0.0, hsv_h=0.015, hsv_s=0.7, hsv_v=0.4,
               fliplr=0.5, flipud=0.0, device_augment=False)
    base = get_cfg({})
    assert {k: base[k] for k in ref} == ref  # the reference's names and default values (ultralytics/cfg/default.yaml:33,105-116)
    for bad in (dict(mosaic=1.5), dict(fliplr=-0.1), dict(hsv_h=2), dict(scale=1.01), dict(translate=7), dict(perspective=1.5)):
        with pytest.raises(ValueError):
            get_cfg(bad)
    for bad in (dict(close_mosaic=1.5), dict(device_augment="yes"), dict(degrees="ten"), dict(mosaic=True)):
        with pytest.raises(TypeError):
            get_cfg(bad)
    assert get_cfg(dict(degrees=10, shear=2.5))["degrees"] == 10  # int or float, no range
    for unknown in (dict(mixup=0.1), dict(copy_paste=0.1), dict(auto_augment="randaugment"), dict(erasing=0.4)):
        with pytest.raises(KeyError):
            get_cfg(unknown)


def _toy_dataset(n=12, s=32, seed=3):
    g = np.random.default_rng(seed)
    counts = g.integers(0, 6, n)
    m = int(counts.sum())
    return dict(img=g.integers(0, 256, (n, 3, s, s), dtype=np.uint8), batch_idx=np.repeat(np.arange(n), counts).astype(np.float32),
                cls=g.integers(0, 10, (m, 1)).astype(np.float32),
                bboxes=np.concatenate((g.uniform(0.2, 0.8, (m, 2)), g.uniform(0.1, 0.4, (m, 2))), 1).astype(np.float32)), counts


def test_device_augment_draws_do_not_depend_on_the_batching():
    from drone_yolo_amd.engine.trainer import TensorLoader, get_cfg

    data, counts = _toy_dataset()
    args = get_cfg(dict(device_augment=True, degrees=5.0, shear=2.0, perspective=0.0005, flipud=0.3))
    aug = A.DeviceAugment(args, 32, data, seed=7)
    assert aug.label_bound() == 4 * int(counts.max())
    tdata = {k: torch.from_numpy(v) for k, v in data.items()}

    def per_sample(batch, world):
        out = {}
        for rank in range(world):
            ld = TensorLoader(tdata, batch, rank, world, seed=7)
            ld.set_epoch(2)
            idx = ld.indices()
            for s in range(0, len(idx), batch):
                take = idx[s : s + batch]
                table, lab = aug.build(2, take)
                for j, i in enumerate(take):
                    rows = lab["batch_idx"] == j
                    out[i] = (table[j].tobytes(), lab["cls"][rows].tobytes(), lab["bboxes"][rows].tobytes())
        return out

    a, b, c = per_sample(4, 1), per_sample(16, 1), per_sample(4, 2)
    assert set(a) == set(range(12)) and a == b and a == c
    t2, _ = aug.build(2, list(range(12)))
    t3, _ = aug.build(3, list(range(12)))
    assert all(t2[i].tobytes() != t3[i].tobytes() for i in range(12))  # another epoch, another draw
    assert set(np.unique(t2["n_src"])) <= {1, 4} and t2.dtype.itemsize == ctypes.sizeof(A._lib.AugRow)
    off, _ = aug.build(2, list(range(12)), mosaic_on=False)  # close_mosaic: the four-image branch off, the rest of the draw unchanged
    assert (off["n_src"] == 1).all() and np.array_equal(off["hsv"], t2["hsv"]) and np.array_equal(off["flags"], t2["flags"])
    _, lab = aug.build(2, list(range(12)))
    assert lab["bboxes"].min() >= 0.0 and lab["bboxes"].max() <= 1.0 and lab["cls"].shape[1] == 1 and lab["bboxes"].dtype == np.float32
    # a sample beyond the step's row limit is refused by name
    big = dict(data)
    big["batch_idx"] = np.zeros(A.MAX_LABEL_ROWS + 1, dtype=np.float32)
    big["cls"] = np.zeros((A.MAX_LABEL_ROWS + 1, 1), dtype=np.float32)
    big["bboxes"] = np.tile(np.array([[0.5, 0.5, 0.3, 0.3]], dtype=np.float32), (A.MAX_LABEL_ROWS + 1, 1))
    still = get_cfg(dict(device_augment=True, mosaic=0.0, scale=0.0, translate=0.0))
    with pytest.raises(ValueError, match="sample 0 .* label rows"):
        A.DeviceAugment(still, 32, big, seed=0).build(0, [0])


def test_dataset_yaml_loader(tmp_path):
    from PIL import Image

    from drone_yolo_amd.engine.trainer import load_dataset

    with pytest.raises(FileNotFoundError, match="missing.yaml"):
        load_dataset(str(tmp_path / "missing.yaml"), 32, 10, 0)
    rng = np.random.default_rng(0)
    shapes = {"train": [(24, 32), (32, 16), (40, 64)], "val": [(32, 32), (10, 20)]}
    for split, hw in shapes.items():
        (tmp_path / "images" / split).mkdir(parents=True)
        (tmp_path / "labels" / split).mkdir(parents=True)
        for i, (h, w) in enumerate(hw):
            Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(tmp_path / "images" / split / f"im{i}.png")
            if i != 1:  # im1 has no label file: a background image
                (tmp_path / "labels" / split / f"im{i}.txt").write_text("3 0.5 0.5 0.5 0.25\n1 0.25 0.75 0.1 0.2\n")
    (tmp_path / "data.yaml").write_text(f"path: {tmp_path}\ntrain: images/train\nval: images/val\nnames:\n  0: a\n  1: b\n  2: c\n  3: d\n")
    d = load_dataset(str(tmp_path / "data.yaml"), 32, 4, 0)
    assert d["img"].dtype == torch.uint8 and tuple(d["img"].shape) == (3, 3, 32, 32) and tuple(d["val"]["img"].shape) == (2, 3, 32, 32)
    assert d["rect"].dtype == torch.int32 and d["rect"].tolist() == [[4, 0, 24, 32], [0, 8, 32, 16], [6, 0, 20, 32]]  # (top, left, h, w); im2 halved
    assert d["val"]["rect"].tolist() == [[0, 0, 32, 32], [8, 0, 16, 32]]  # im1 of val doubled: the long side becomes imgsz
    img = d["img"].numpy()
    assert (img[0, :, :4] == 114).all() and (img[0, :, 28:] == 114).all() and (img[1, :, :, :8] == 114).all() and (img[1, :, :, 24:] == 114).all()
    src0 = np.asarray(Image.open(tmp_path / "images" / "train" / "im0.png"))
    assert np.array_equal(img[0, :, 4:28], src0.transpose(2, 0, 1))  # unresized: the pixels themselves, RGB
    assert d["batch_idx"].tolist() == [0, 0, 2, 2] and d["cls"].view(-1).tolist() == [3, 1, 3, 1]
    exp0 = np.array([[0.5, (0.5 * 24 + 4) / 32, 0.5, 0.25 * 24 / 32], [0.25, (0.75 * 24 + 4) / 32, 0.1, 0.2 * 24 / 32]], dtype=np.float32)
    assert np.allclose(d["bboxes"][:2].numpy(), exp0, atol=1e-6)
    assert d["val"]["batch_idx"].tolist() == [0, 0] and d["names"] == {0: "a", 1: "b", 2: "c", 3: "d"}
    # and the augmentation side reads the valid region only: a mosaic of these pastes (h, w) = rect's size
    from drone_yolo_amd.engine.trainer import get_cfg

    aug = A.DeviceAugment(get_cfg(dict(device_augment=True)), 32, {k: d[k].numpy() for k in ("img", "batch_idx", "cls", "bboxes", "rect")}, seed=1)
    assert aug._labels_of(0)[2] == (24, 32) and np.allclose(aug._labels_of(0)[1], [[0.5, 0.5, 0.5, 0.25], [0.25, 0.75, 0.1, 0.2]], atol=1e-6)


def test_augment_entry_point_validates_without_gpu():
    import drone_yolo_amd._lib as L

    h = L.lib()
    buf = (ctypes.c_uint8 * 256)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert h.dy_augment_u8_nchw(None, p, p, 1, 8, 8, 1, 8, None) == -1 and b"null" in h.dy_last_error_string()
    assert h.dy_augment_u8_nchw(p, None, p, 1, 8, 8, 1, 8, None) == -1 and h.dy_augment_u8_nchw(p, p, None, 1, 8, 8, 1, 8, None) == -1
    assert h.dy_augment_u8_nchw(p, p, p, 1, 8, 8, 1, 6, None) == -1 and b"multiple of 4" in h.dy_last_error_string()
    for bad in ((0, 8, 8, 1, 8), (1, 0, 8, 1, 8), (1, 8, -1, 1, 8), (1, 8, 8, 0, 8), (1, 8, 8, 1, 0)):
        assert h.dy_augment_u8_nchw(p, p, p, *bad, None) == -1


def test_augment_struct_layout_matches_header(tmp_path):
    import drone_yolo_amd._lib as L

    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dyolo.h"\nint main(){printf("%zu %zu %zu %zu %zu\\n", sizeof(dy_aug_src), '
                   "sizeof(dy_aug_row), offsetof(dy_aug_row, src), offsetof(dy_aug_row, minv), offsetof(dy_aug_row, hsv));return 0;}\n")
    exe = tmp_path / "s"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert sizes == [ctypes.sizeof(L.AugSrc), ctypes.sizeof(L.AugRow), L.AugRow.src.offset, L.AugRow.minv.offset, L.AugRow.hsv.offset]
    assert A.AUG_ROW_DTYPE.itemsize == sizes[1] and [A.AUG_ROW_DTYPE.fields[k][1] for k in ("src", "minv", "hsv")] == sizes[2:]


def write_yolo_folder(root, shapes, seed=0, ncls=4):
    """A YOLO-format dataset under ``root`` (images/<split>, labels/<split>, data.yaml); every second image of a split has labels."""
    from PIL import Image

    rng = np.random.default_rng(seed)
    for split, hw in shapes.items():
        (root / "images" / split).mkdir(parents=True)
        (root / "labels" / split).mkdir(parents=True)
        for i, (h, w) in enumerate(hw):
            Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(root / "images" / split / f"im{i}.png")
            if i % 2 == 0:
                (root / "labels" / split / f"im{i}.txt").write_text(f"{i % ncls} 0.5 0.5 0.5 0.4\n{(i + 1) % ncls} 0.3 0.7 0.3 0.35\n")
    names = "".join(f"  {k}: c{k}\n" for k in range(ncls))
    (root / "data.yaml").write_text(f"path: {root}\ntrain: images/train\nval: images/val\nnames:\n{names}")
    return str(root / "data.yaml")


def test_trainer_takes_a_dataset_yaml_from_the_public_interface(tmp_path, monkeypatch):
    """DetectionTrainer's argument check lets an existing dataset YAML through (it is decoded when training is set up): without a GPU the
    construction gets as far as the 'no CPU fallback' error, not a complaint about the dataset; a missing YAML is refused by name."""
    import drone_yolo_amd.engine.trainer as T

    path = write_yolo_folder(tmp_path, {"train": [(24, 32), (32, 16)], "val": [(32, 32)]})
    assert T.load_dataset(path, 0, 0, 0) == {}
    ov = dict(model="yolov8n-p2-repvgg.yaml", nc=4, data=path, imgsz=32, device_augment=True, project=str(tmp_path), name="r")
    if torch.cuda.is_available():
        assert T.DetectionTrainer(overrides=ov).args["data"] == path
    else:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            T.DetectionTrainer(overrides=ov)
    for exc in (FileNotFoundError, NotImplementedError):
        with pytest.raises(exc, match="nothing.yaml"):
            T.DetectionTrainer(overrides=dict(ov, data=str(tmp_path / "nothing.yaml")))
    # augmentation arguments without device_augment: one line says they have no effect
    lines = []
    monkeypatch.setattr(T.LOGGER, "info", lambda m, *a, **k: lines.append(str(m)))
    try:
        T.DetectionTrainer(overrides=dict(model="yolov8n-p2-repvgg.yaml", nc=4, data="synthetic:4", imgsz=32, mosaic=0.5, fliplr=0.0, project=str(tmp_path), name="q"))
    except RuntimeError:
        pass  # (no GPU here)
    said = [m for m in lines if "no effect without device_augment" in m]
    assert len(said) == 1 and "fliplr" in said[0] and "mosaic" in said[0]
    lines.clear()
    try:
        T.DetectionTrainer(overrides=dict(ov, data="synthetic:4"))
    except RuntimeError:
        pass
    assert not [m for m in lines if "no effect" in m]


def test_dataset_yaml_larger_than_host_memory_is_refused_with_its_size(tmp_path, monkeypatch):
    import drone_yolo_amd.engine.trainer as T

    path = write_yolo_folder(tmp_path, {"train": [(24, 32), (32, 16)], "val": [(32, 32)]})
    monkeypatch.setattr(T, "_host_memory_available", lambda: 2 * 3 * 32 * 32 * 2 - 2)  # half of it: one byte short of the two training images
    with pytest.raises(MemoryError, match=r"2 images = 0\.00 GiB .*32 x 32"):
        T.load_dataset(path, 32, 4, 0)
    monkeypatch.setattr(T, "_host_memory_available", lambda: 2 * 3 * 32 * 32 * 2)  # the training split fits exactly, nothing is left for val
    with pytest.raises(MemoryError, match="'val' holds 1 images"):
        T.load_dataset(path, 32, 4, 0)
