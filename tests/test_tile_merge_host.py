"""CPU: ``dy_tile_merge`` / ``dy_tiles_batch_u8_to_nchw_f32`` check their arguments before any HIP call; the seeded rows the GPU tests
merge (tests/_tile_util.py) keep clear of the merge thresholds by construction; the numpy restatement ``merge_ref`` has the properties the
two metrics are there for; the predictor refuses bad tile arguments before it touches a device."""
import ctypes
import os

import numpy as np
import pytest

from tests._tile_util import CASES, IOS_THR, IOU_THR, MARGIN, SEEDS, frame_boxes, merge_ref, pair_measures, tile_rows
from tests._util import ROOT, load_yaml

def _desc(L, **kw):
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    d = L.TileMergeDesc()
    d.rows = d.counts = d.offsets_yx = d.out = d.out_count = d.out_index = d.workspace = p
    d.frames, d.tiles, d.max_det, d.nc, d.frame_h, d.frame_w = 1, 2, 4, 3, 64, 64
    d.thr, d.metric, d.agnostic, d.merge_max_det, d.workspace_bytes = 0.6, 0, 0, 8, 1 << 30
    for k, v in kw.items():
        setattr(d, k, v)
    d._keep = buf
    return d


def test_entry_points_refuse_bad_arguments_without_a_device():
    import drone_yolo_amd._lib as L

    h = L.lib()
    assert h.dy_tile_merge(None, None) == -1
    assert h.dy_tile_merge(ctypes.byref(L.TileMergeDesc()), None) == -1 and b"null" in h.dy_last_error_string()
    for name in ("rows", "counts", "offsets_yx", "out", "out_count", "workspace"):
        assert h.dy_tile_merge(ctypes.byref(_desc(L, **{name: None})), None) == -1 and b"null" in h.dy_last_error_string(), name
    assert h.dy_tile_merge(ctypes.byref(_desc(L, tiles=32769, max_det=1)), None) == -2 and b"32768" in h.dy_last_error_string()  # DY_ERR_UNSUPPORTED
    assert h.dy_tile_merge(ctypes.byref(_desc(L, tiles=10923, max_det=3)), None) == -2  # 32769 slots
    assert h.dy_tile_merge(ctypes.byref(_desc(L, merge_max_det=4097)), None) == -2 and b"4096" in h.dy_last_error_string()
    assert h.dy_tile_merge(ctypes.byref(_desc(L, metric=2)), None) == -1 and b"metric" in h.dy_last_error_string()
    for kw in (dict(frames=0), dict(tiles=0), dict(max_det=0), dict(nc=0), dict(frame_h=0), dict(merge_max_det=0), dict(thr=1.5)):
        assert h.dy_tile_merge(ctypes.byref(_desc(L, **kw)), None) == -1, kw
    assert h.dy_tile_merge(ctypes.byref(_desc(L, workspace_bytes=8)), None) == -4  # DY_ERR_WORKSPACE
    assert h.dy_tile_merge_workspace_bytes(2, 8, 300) == 2 * 4096 * 8 and h.dy_tile_merge_workspace_bytes(1, 109, 300) == 32768 * 8
    assert h.dy_tile_merge_workspace_bytes(1, 110, 300) == -1 and h.dy_tile_merge_workspace_bytes(0, 1, 1) == -1
    p = _desc(L).rows
    assert h.dy_tiles_batch_u8_to_nchw_f32(None, p, p, 1, 1, 8, 8, 8, 8, 1, 114.0, None) == -1 and b"null" in h.dy_last_error_string()
    assert h.dy_tiles_batch_u8_to_nchw_f32(p, p, p, 0, 1, 8, 8, 8, 8, 1, 114.0, None) == -1 and b"dims" in h.dy_last_error_string()


def test_descriptor_mirror_matches_header():
    import subprocess
    import tempfile

    import drone_yolo_amd._lib as L

    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "s.c")
        open(src, "w").write('#include <stdio.h>\n#include <stddef.h>\n#include "dyolo.h"\nint main(){printf("%zu %zu %zu %zu\\n", sizeof(dy_tile_merge_desc), '
                             "offsetof(dy_tile_merge_desc, frames), offsetof(dy_tile_merge_desc, thr), offsetof(dy_tile_merge_desc, out));return 0;}\n")
        exe = os.path.join(td, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    D = L.TileMergeDesc
    assert got == [ctypes.sizeof(D), D.frames.offset, D.thr.offset, D.out.offset]


@pytest.mark.parametrize("name", list(CASES))
def test_generated_rows_keep_clear_of_the_thresholds(name):
    """In float64: boxes of different objects cannot overlap (each lies inside its object's lattice cells, and no two objects share a cell); of
    the pairs inside an object none has an IoU within 0.02 of 0.6 or an IoS within 0.02 of 0.8.  (The margin covers the parent chain's
    cls * 7680 coordinate offset, up to 2^-7 px per coordinate on boxes a few pixels wide.)"""
    F, K, md, nc, hw, tile, ov = CASES[name]
    rows, counts, offs, obj, cuts, cell = tile_rows(SEEDS[name], F, K, md, nc, hw, tile, ov, with_meta=True)
    assert rows.shape == (F * K, md, 6) and rows.dtype == np.float32 and counts.shape == (F * K,) and offs.shape == (K, 2)
    assert (rows[..., :4] >= 0).all() and (rows[..., :4] <= tile).all() and not rows[np.arange(md)[None, :] >= counts[:, None]].any()
    if K > 1:
        assert counts.min() == 0 and counts.max() == md and len(set(counts.tolist())) > 3  # ragged, with both ends
    n_pairs = n_ties = 0
    for f in range(F):
        box, cls, tl, rr = frame_boxes(rows, counts, offs, f, K)
        o, c = obj[f * K + tl, rr], cell[f * K + tl, rr]
        assert (o >= 0).all()
        if len(o) == 0:
            continue
        assert (box[:, 0] >= c[:, 0]).all() and (box[:, 1] >= c[:, 1]).all() and (box[:, 2] <= c[:, 2]).all() and (box[:, 3] <= c[:, 3]).all()
        pitch = c[0, 3] - c[0, 1]
        owner = {}
        for oi, cc in {int(a): tuple(b) for a, b in zip(o, c)}.items():  # the unit cells an object owns are its alone
            for ix in range(int(round(cc[0] / pitch)), int(round(cc[2] / pitch))):
                assert owner.setdefault((ix, int(round(cc[1] / pitch))), oi) == oi
        order = np.argsort(o, kind="stable")
        so = o[order]
        for d in range(1, 12):  # an object has at most a handful of views: all pairs (i, i + d) of the rows sorted by object
            same = so[d:] == so[:-d]
            if not same.any():
                break
            a, b = order[:-d][same], order[d:][same]
            iou, ios = pair_measures(box[a], box[b])
            assert (np.abs(iou - IOU_THR) >= MARGIN).all() and (np.abs(ios - IOS_THR) >= MARGIN).all()
            whole = (iou > 0.85)
            assert (whole | ((iou > 0.3) & (iou < 0.5) & (ios >= 0.95))).all()  # duplicates, or a clipped part against its whole box
            n_pairs += len(a)
        else:
            raise AssertionError("an object with 12 or more views")
        sc = rows[f * K + tl, rr, 4]
        n_ties += len(sc) - len(np.unique(sc))
    if K > 1:
        assert n_pairs > 0 and n_ties > 0 and sum(len(c) for c in cuts) >= 3


def test_merge_ref_iou_keeps_cut_objects_twice_ios_once():
    F, K, md, nc, hw, tile, ov = CASES["lds"]
    rows, counts, offs, obj, cuts, _ = tile_rows(SEEDS["lds"], F, K, md, nc, hw, tile, ov, with_meta=True)
    per = {}
    for metric, thr in ((0, IOU_THR), (1, IOS_THR)):
        out, cnt, idx = merge_ref(rows, counts, offs, hw, thr, metric, False, 4096)
        assert (cnt < 4096).all() and cnt[0] > 0 and cnt[1] == 0 and cnt[2] > 0  # (the middle frame has no rows)
        for f in range(F):
            slots = idx[f, : cnt[f]]
            assert (idx[f, cnt[f] :] == -1).all() and not out[f, cnt[f] :].any() and len(set(slots.tolist())) == cnt[f]
            assert (np.diff(out[f, : cnt[f], 4]) <= 0).all()  # descending score
            kept_obj = obj[f * K + slots // md, slots % md]
            n_kept = np.bincount(kept_obj, minlength=int(obj.max()) + 1)
            want = 2 if metric == 0 else 1
            assert all(n_kept[o] == want for o in cuts[f]), (metric, [int(n_kept[o]) for o in cuts[f]])
        per[metric] = cnt
    assert (per[1][[0, 2]] < per[0][[0, 2]]).all()
    out, cnt, idx = merge_ref(rows, counts, offs, hw, IOS_THR, 1, True, 4096)  # agnostic IoS: one box per object
    for f in (0, 2):
        slots = idx[f, : cnt[f]]
        assert np.bincount(obj[f * K + slots // md, slots % md]).max() == 1 and cnt[f] < per[1][f]


def test_merge_ref_truncates_and_ties_go_to_the_lower_slot():
    rows = np.zeros((2, 3, 6), np.float32)
    rows[0, :2] = [[10, 10, 20, 20, 0.5, 1], [40, 40, 50, 50, 0.5, 1]]
    rows[1, :3] = [[0, 10, 10, 20, 0.5, 1], [30, 30, 40, 40, 0.5, 0], [50, 50, 60, 60, 0.9, 1]]  # tile 1 at x = 10: its first row duplicates slot 0
    counts, offs = np.array([2, 3], np.int32), np.array([[0, 0], [0, 10]], np.int32)
    out, cnt, idx = merge_ref(rows, counts, offs, (64, 64), 0.6, 0, False, 8)
    assert cnt[0] == 4 and idx[0, :4].tolist() == [5, 0, 1, 4] and out[0, 0].tolist() == [60.0, 50.0, 64.0, 60.0, np.float32(0.9), 1.0]  # clamped to the frame
    out, cnt, idx = merge_ref(rows, counts, offs, (64, 64), 0.6, 0, False, 2)
    assert cnt[0] == 2 and idx[0].tolist() == [5, 0]


def test_predictor_refuses_bad_tile_arguments_before_device_work():
    import drone_yolo_amd as D

    model = D.DetectionModel(dict(load_yaml("yolov8-p2-repvgg.yaml", "n", 10)), nc=10, verbose=False)
    P = D.engine.predictor.DetectionPredictor
    with pytest.raises(ValueError, match="multiple of the model's largest stride"):
        P(model, dict(tile=100, device="cpu"))
    with pytest.raises(ValueError, match="merge_metric"):
        P(model, dict(tile=128, merge_metric="giou", device="cpu"))
    with pytest.raises(NotImplementedError, match="augment"):
        P(model, dict(tile=128, augment=True, device="cpu"))
    yolo = D.YOLO("yolov8n-p2-repvgg.yaml")
    with pytest.raises(ValueError, match="1024"):
        yolo.track([np.zeros((64, 64, 3), np.uint8)], tile=128, merge_max_det=1025, device="cpu")
