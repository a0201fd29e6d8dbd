"""Writes tests/golden/train_aug.npz: what the REAL reference's augmentation code computes on small inputs, for
tests/test_augment_host.py and tests/test_augment_gpu.py.

    python tools/make_aug_golden.py

The reference is imported through oracle/make_golden.py::import_reference (a stub ``cv2``; nothing under oracle/ changes).  With that stub
``Mosaic._mosaic4``, ``RandomPerspective.apply_bboxes`` / ``box_candidates``, ``RandomFlip`` and ``Instances`` run as they are (numpy).
For the whole ``RandomPerspective.__call__`` the stub gets a ``getRotationMatrix2D`` (the closed form for centre (0, 0)) and a
``warpAffine`` / ``warpPerspective`` that hand the image back: the reference's own label path then runs end to end and returns M; the pixels
of that call are not recorded.  The reference draws from the global ``random`` module; the draws are preset here by giving its augment
module a ``random`` whose ``uniform`` / ``random`` replay a list.  Only arrays go into the file.
"""
from __future__ import annotations

import math
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

S = 64
SHAPES = [(48, 64), (64, 48), (40, 64), (64, 64), (64, 30), (56, 64)]  # (h, w): long side S or smaller
# (yc, xc) and the four images: centred, corners of the range (grey borders), off-centre, small images
MOSAICS = [((64, 64), (0, 1, 2, 3)), ((32, 32), (3, 0, 5, 1)), ((95, 95), (1, 2, 3, 4)), ((40, 90), (4, 4, 0, 2)), ((90, 33), (2, 5, 1, 0)),
           ((64, 100), (5, 3, 4, 1)), ((77, 50), (0, 0, 0, 0))]
# draws of affine_transform in its order: perspective x, y; angle; scale; shear x, y (degrees); translation x, y (fractions of S)
PERSP = {
    "identity": (0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 1.0),
    "shift_centre": (0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.5, 0.5),
    "shift_17_40": (0.0, 0.0, 0.0, 1.0, 0.0, 0.0, (64 - 17) / 64, (64 - 40) / 64),
    "scale_0.5": (0.0, 0.0, 0.0, 0.5, 0.0, 0.0, 0.55, 0.45),
    "scale_1.5": (0.0, 0.0, 0.0, 1.5, 0.0, 0.0, 0.5, 0.58),
    "rotate": (0.0, 0.0, 10.0, 1.1, 0.0, 0.0, 0.47, 0.52),
    "shear": (0.0, 0.0, 0.0, 0.9, 5.0, -3.0, 0.5, 0.5),
    "perspective": (0.0005, -0.0003, -4.0, 0.8, 1.0, 2.0, 0.52, 0.5),
}


class Replay:
    """Stands in for the ``random`` module inside the reference's augment module: ``uniform`` / ``random`` return preset values."""

    def __init__(self):
        self.values = []

    def load(self, values):
        self.values = list(values)

    def uniform(self, a, b):
        return self.values.pop(0)

    def random(self):
        return self.values.pop(0)


def main() -> None:
    from oracle.make_golden import import_reference

    import_reference()
    import cv2  # the stub
    from ultralytics.data import augment as raug
    from ultralytics.utils.instance import Instances as RefInstances

    def Instances(bboxes, bbox_format, normalized):  # boxes only: the empty segment array a detection dataset carries (data/dataset.py)
        return RefInstances(bboxes, np.zeros((0, 1000, 2), dtype=np.float32), None, bbox_format=bbox_format, normalized=normalized)

    def rot(angle, center, scale):
        assert tuple(center) == (0, 0)
        al, be = scale * math.cos(math.radians(angle)), scale * math.sin(math.radians(angle))
        return np.array([[al, be, 0.0], [-be, al, 0.0]], dtype=np.float64)

    cv2.getRotationMatrix2D = rot
    cv2.warpAffine = lambda img, m, dsize=None, borderValue=None: img
    cv2.warpPerspective = lambda img, m, dsize=None, borderValue=None: img
    replay = Replay()
    raug.random = replay

    rng = np.random.default_rng(20240)
    out = {"S": np.int64(S)}
    imgs, labs = [], []
    for i, (h, w) in enumerate(SHAPES):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        n = int(rng.integers(3, 9))
        cxy = rng.uniform(0.05, 0.95, (n, 2))
        wh = rng.uniform(0.04, 0.6, (n, 2))
        lab = np.concatenate((rng.integers(0, 10, (n, 1)).astype(np.float64), cxy, wh), 1).astype(np.float32)
        imgs.append(img), labs.append(lab)
        out[f"img_{i}"], out[f"lab_{i}"] = img, lab
    out["n_img"] = np.int64(len(SHAPES))

    def patch(i):
        h, w = SHAPES[i]
        return {"img": imgs[i], "resized_shape": (h, w), "ori_shape": (h, w), "im_file": str(i), "cls": labs[i][:, :1].copy(),
                "instances": Instances(labs[i][:, 1:].copy(), bbox_format="xywh", normalized=True)}

    # ---- Mosaic._mosaic4: canvas, concatenated labels, and the (padw, padh) it hands to _update_labels
    mosaic = object.__new__(raug.Mosaic)
    mosaic.imgsz, mosaic.border, mosaic.n = S, (-S // 2, -S // 2), 4
    pads = []
    real_update = raug.Mosaic._update_labels

    def spy_update(labels, padw, padh):
        pads.append((padw, padh))
        return real_update(labels, padw, padh)

    mosaic._update_labels = spy_update
    out["n_mosaic"] = np.int64(len(MOSAICS))
    first = None
    for k, ((yc, xc), ids) in enumerate(MOSAICS):
        pads.clear()
        replay.load([yc + 0.5, xc + 0.5])  # int(uniform(...)) truncates
        lb = patch(ids[0])
        lb["mix_labels"] = [patch(i) for i in ids[1:]]
        res = mosaic._mosaic4(lb)
        assert res["img"].shape == (2 * S, 2 * S, 3)
        out[f"mos{k}_center"], out[f"mos{k}_ids"] = np.array([yc, xc], dtype=np.int64), np.array(ids, dtype=np.int64)
        out[f"mos{k}_canvas"] = res["img"]
        out[f"mos{k}_cls"], out[f"mos{k}_boxes"] = res["cls"].astype(np.float32), res["instances"].bboxes.astype(np.float32)
        out[f"mos{k}_pads"] = np.array(pads, dtype=np.int64)
        assert res["instances"].bboxes.dtype == np.float32
        if first is None:
            first = (res["img"], out[f"mos{k}_cls"].copy(), out[f"mos{k}_boxes"].copy())

    # ---- RandomPerspective.__call__ on mosaic 0's canvas and labels (mosaic_border = -S/2), and once on a plain image (no mosaic)
    names = list(PERSP)
    out["persp_names"] = np.array(names)
    for name in names:
        draws = PERSP[name]
        for tag, make in (("m", lambda: {"img": first[0], "cls": first[1].copy(), "mosaic_border": (-S // 2, -S // 2),
                                         "instances": Instances(first[2].copy(), bbox_format="xyxy", normalized=False)}),
                          ("p", lambda: {"img": imgs[3], "cls": labs[3][:, :1].copy(),
                                         "instances": Instances(labs[3][:, 1:].copy(), bbox_format="xywh", normalized=True)})):
            rp = raug.RandomPerspective(degrees=1.0, translate=0.1, scale=0.5, shear=1.0, perspective=abs(draws[0]), pre_transform=None)
            seen = {}
            real_affine, real_cand = rp.affine_transform, raug.RandomPerspective.box_candidates

            def spy_affine(img, border, _f=real_affine, _s=seen):
                img, m, s = _f(img, border)
                _s["M"], _s["scale"] = m, s
                return img, m, s

            def spy_cand(box1, box2, area_thr=0.1, _f=real_cand, _s=seen, **kw):
                keep = _f(box1=box1, box2=box2, area_thr=area_thr, **kw)
                _s["keep"], _s["new"], _s["before"], _s["area_thr"] = keep, box2.T.copy(), box1.T.copy(), area_thr
                return keep

            rp.affine_transform, rp.box_candidates = spy_affine, spy_cand
            replay.load(draws)
            lb = make()
            if tag == "p" and name not in ("identity", "rotate", "scale_0.5"):
                continue
            res = rp(lb)
            assert seen["area_thr"] == 0.10 and seen["M"].dtype == np.float32
            key = f"persp_{tag}_{name}"
            out[f"{key}_draws"] = np.array(draws, dtype=np.float64)
            out[f"{key}_M"], out[f"{key}_scale"] = seen["M"], np.float64(seen["scale"])
            out[f"{key}_new"], out[f"{key}_keep"] = seen["new"].astype(np.float32), seen["keep"]
            out[f"{key}_out_boxes"], out[f"{key}_out_cls"] = res["instances"].bboxes.astype(np.float32), res["cls"].astype(np.float32)

    # ---- RandomFlip (vertical, then horizontal) followed by Format's normalisation, on the labels the centred shift keeps
    base = out["persp_m_shift_centre_out_boxes"]
    out["flip_in"] = base
    for tag, ud, lr in (("none", False, False), ("ud", True, False), ("lr", False, True), ("both", True, True)):
        lb = {"img": np.zeros((S, S, 3), dtype=np.uint8), "instances": Instances(base.copy(), bbox_format="xyxy", normalized=False)}
        replay.load([0.0 if ud else 1.0])
        lb = raug.RandomFlip(p=0.5, direction="vertical")(lb)
        replay.load([0.0 if lr else 1.0])
        lb = raug.RandomFlip(p=0.5, direction="horizontal")(lb)
        inst = lb["instances"]
        inst.convert_bbox(format="xywh")
        inst.normalize(S, S)
        out[f"flip_{tag}"] = inst.bboxes.astype(np.float32)

    dst = ROOT / "tests" / "golden" / "train_aug.npz"
    np.savez_compressed(dst, **out)
    print(f"wrote {dst} ({dst.stat().st_size} bytes, {len(out)} arrays)")


if __name__ == "__main__":
    main()
