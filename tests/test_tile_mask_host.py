"""CPU: the references of the tiled-segmentation tests hold what the GPU tests rely on (``owner_ref`` agrees with ``fuse_ref``; the float64
mask reference is decisive on all but a sliver of the pixels), ``dy_tile_mask_owner`` / ``dy_tile_process_mask`` check their arguments before
any HIP call, and ``YOLO.predict`` refuses what a segmentation model does not take before a predictor is built."""
import ctypes

import numpy as np
import pytest
import torch

from tests._fuse_util import fuse_ref
from tests._tile_mask_util import CASES, STRIDES, case_reference, owner_histogram, owner_ref
from tests._tile_util import CASES as MERGE_CASES
from tests._tile_util import IOS_THR, IOU_THR, SEEDS, tile_rows


@pytest.mark.parametrize("name", ["one_tile", "lds", "4k"])
def test_owner_ref_histogram_is_fuse_ref_members(name):
    F, K, md, nc, hw, tile, ov = MERGE_CASES[name]
    rows, counts, offs = tile_rows(SEEDS[name], F, K, md, nc, hw, tile, ov)
    for metric, agnostic in ((0, False), (1, True)):
        thr = IOS_THR if metric else IOU_THR
        owner, (_, cnt, idx) = owner_ref(rows, counts, offs, hw, thr, metric, agnostic, 1000, stitch=True)
        _, fcnt, fidx, members = fuse_ref(rows, counts, offs, hw, thr, metric, agnostic, 1000, "union")
        assert np.array_equal(cnt, fcnt) and np.array_equal(idx, fidx)
        assert np.array_equal(owner_histogram(owner, 1000), members)
        plain, _ = owner_ref(rows, counts, offs, hw, thr, metric, agnostic, 1000, stitch=False)
        assert np.array_equal(owner_histogram(plain, 1000), (members > 0).astype(np.int32))
        assert np.array_equal(plain >= 0, (owner >= 0) & (plain == owner))  # the kept slots are the same, with the same row


@pytest.mark.parametrize("s", STRIDES)
def test_reference_is_decisive(s):
    """The unsure share of the float64 reference alone, pooled over the cases of a stride: at most 1e-3 (the project's cap for
    ``dy_process_mask``) of at least 50,000 in-box pixels."""
    unsure = inbox = 0
    for name in CASES:
        _, (ref, uns, inb) = case_reference(name, s)
        unsure += int((uns & inb).sum())
        inbox += int(inb.sum())
    print(f"stride {s}: {unsure} unsure of {inbox} in-box pixels")
    assert inbox >= 50000
    assert unsure / inbox <= 1e-3


def test_entry_points_validate_without_gpu():
    import drone_yolo_amd._lib as L

    h = L.lib()
    buf = (ctypes.c_float * 1024)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def owner_desc(**kw):
        d = L.TileMaskOwnerDesc()
        d.rows = d.counts = d.offsets_yx = d.kept_index = d.kept_count = d.owner = p
        d.frames, d.tiles, d.max_det, d.merge_max_det, d.thr, d.metric, d.agnostic, d.stitch = 1, 2, 8, 16, 0.6, 0, 0, 1
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    assert h.dy_tile_mask_owner(None, None) == -1
    for name in ("rows", "counts", "offsets_yx", "kept_index", "kept_count", "owner"):
        assert h.dy_tile_mask_owner(ctypes.byref(owner_desc(**{name: None})), None) == -1 and b"null" in h.dy_last_error_string(), name
    assert h.dy_tile_mask_owner(ctypes.byref(owner_desc(tiles=32769, max_det=1)), None) == -2 and b"32768" in h.dy_last_error_string()
    assert h.dy_tile_mask_owner(ctypes.byref(owner_desc(merge_max_det=4097)), None) == -2 and b"4096" in h.dy_last_error_string()
    assert h.dy_tile_mask_owner(ctypes.byref(owner_desc(metric=2)), None) == -1 and b"metric" in h.dy_last_error_string()
    for kw in (dict(frames=0), dict(tiles=0), dict(max_det=0), dict(merge_max_det=0), dict(thr=1.5), dict(thr=-0.1)):
        assert h.dy_tile_mask_owner(ctypes.byref(owner_desc(**kw)), None) == -1, kw

    def mask_desc(**kw):
        d = L.TileProcessMaskDesc()
        d.protos = d.side = d.counts = d.offsets_yx = d.owner = d.dest = d.out = p
        d.frames, d.tiles, d.max_det, d.merge_max_det, d.nm, d.mh, d.mw, d.ld_p = 1, 2, 8, 16, 32, 16, 16, 32
        d.tile_h, d.tile_w, d.frame_h, d.frame_w, d.stride, d.total = 64, 64, 64, 100, 1, 3
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    assert h.dy_tile_process_mask(None, None) == -1
    for name in ("protos", "side", "counts", "offsets_yx", "owner", "dest"):
        assert h.dy_tile_process_mask(ctypes.byref(mask_desc(**{name: None})), None) == -1 and b"null" in h.dy_last_error_string(), name
    assert h.dy_tile_process_mask(ctypes.byref(mask_desc(out=None)), None) == -1
    assert h.dy_tile_process_mask(ctypes.byref(mask_desc(stride=3)), None) == -2 and b"stride" in h.dy_last_error_string()  # DY_ERR_UNSUPPORTED
    assert h.dy_tile_process_mask(ctypes.byref(mask_desc(mh=15)), None) == -2 and b"quarter" in h.dy_last_error_string()
    assert h.dy_tile_process_mask(ctypes.byref(mask_desc(tile_w=68)), None) == -2
    assert h.dy_tile_process_mask(ctypes.byref(mask_desc(nm=31)), None) == -2 and b"32" in h.dy_last_error_string()
    assert h.dy_tile_process_mask(ctypes.byref(mask_desc(frame_h=50000, frame_w=50000)), None) == -1  # oh * ow >= 2^31
    assert h.dy_tile_process_mask(ctypes.byref(mask_desc(total=0, out=None)), None) == 0  # DY_OK without a launch


def test_api_refusals_come_before_a_predictor():
    from drone_yolo_amd import YOLO

    y = YOLO("yolov8n-seg.yaml")
    frame = np.zeros((96, 96, 3), np.uint8)
    with pytest.raises(NotImplementedError, match="retina_masks"):
        y.predict([frame], tile=64, retina_masks=True)
    assert y.predictor is None
    with pytest.raises(ValueError, match="tile_mask_stride"):
        y.predict([frame], tile=64, tile_mask_stride=3)
    assert y.predictor is None
    with pytest.raises(NotImplementedError, match="augment"):
        y.predict([frame], tile=64, augment=True)
    assert y.predictor is None
    p2 = YOLO("yolov8n-p2-repvgg-seg.yaml")  # prototypes at half the input: no quarter grid for the frame masks
    with pytest.raises(NotImplementedError, match="tile"):
        p2.predict([frame], tile=64)
    assert p2.predictor is None
    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(NotImplementedError, match="tile"):
        y.predict(x, tile=64)
    with pytest.raises(NotImplementedError, match="track"):
        y.predict(x, mode="track")
    with pytest.raises(NotImplementedError, match="track"):
        y.track(x)
    assert y.predictor is None
