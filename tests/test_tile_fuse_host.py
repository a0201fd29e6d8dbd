"""CPU: ``dy_tile_fuse`` checks its arguments before any HIP call; its descriptor mirror matches the header; the numpy restatement ``fuse_ref``
(tests/_fuse_util.py) keeps what ``merge_ref`` keeps and has the properties the two fusing modes are there for; the predictor refuses a bad
``merge_mode`` before it touches a device."""
import ctypes
import functools
import os

import numpy as np
import pytest

from tests._fuse_util import SPLIT_FRAME, fuse_ref, split_rows
from tests._tile_util import CASES, IOS_THR, IOU_THR, SEEDS, merge_ref, tile_rows
from tests._util import ROOT, load_yaml


def _desc(L, **kw):
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    d = L.TileFuseDesc()
    d.rows = d.counts = d.offsets_yx = d.out = d.out_count = d.out_index = d.out_members = d.workspace = p
    d.frames, d.tiles, d.max_det, d.nc, d.frame_h, d.frame_w = 1, 2, 4, 3, 64, 64
    d.thr, d.metric, d.agnostic, d.merge_max_det, d.mode, d.workspace_bytes = 0.6, 0, 0, 8, 1, 1 << 30
    for k, v in kw.items():
        setattr(d, k, v)
    d._keep = buf
    return d


def test_tile_fuse_refuses_bad_arguments_without_a_device():
    import drone_yolo_amd._lib as L

    h = L.lib()
    call = lambda **kw: h.dy_tile_fuse(ctypes.byref(_desc(L, **kw)), None)  # noqa: E731
    said = lambda word: word in h.dy_last_error_string()  # noqa: E731
    assert h.dy_tile_fuse(None, None) == -1 and said(b"null")
    assert h.dy_tile_fuse(ctypes.byref(L.TileFuseDesc()), None) == -1 and said(b"null")
    for name in ("rows", "counts", "offsets_yx", "out", "out_count", "out_members", "workspace"):
        assert call(**{name: None}) == -1 and said(b"null"), name
    for kw in (dict(frames=0), dict(tiles=0), dict(max_det=0), dict(nc=0), dict(frame_h=0), dict(frame_w=0), dict(merge_max_det=0)):
        assert call(**kw) == -1 and said(b"dims"), kw
    assert call(metric=2) == -1 and said(b"metric")
    for mode in (0, 3, -1):  # 0 is suppression: dy_tile_merge's job
        assert call(mode=mode) == -1 and said(b"mode"), mode
    assert call(thr=1.5) == -1 and said(b"thr") and call(thr=-0.1) == -1 and said(b"thr")
    assert call(tiles=32769, max_det=1) == -2 and said(b"32768")  # DY_ERR_UNSUPPORTED
    assert call(tiles=10923, max_det=3) == -2 and said(b"32768")  # 32769 slots
    assert call(merge_max_det=4097) == -2 and said(b"4096")
    assert call(workspace_bytes=8) == -4 and said(b"workspace")  # DY_ERR_WORKSPACE
    need = h.dy_tile_fuse_workspace_bytes(1, 2, 4, 8)
    assert call(workspace_bytes=need - 1) == -4 and said(b"workspace")
    base = _desc(L)
    assert h.dy_tile_fuse(ctypes.byref(_desc(L, workspace=base.workspace + 8)), None) == -1 and said(b"aligned")
    assert call(mode=2, frame_w=32769) == -2 and said(b"wbf") and call(mode=2, frame_h=32769) == -2 and said(b"wbf")
    # the keys of dy_tile_merge and 40 bytes of accumulators per output row
    assert need == h.dy_tile_merge_workspace_bytes(1, 2, 4) + 8 * 40
    assert h.dy_tile_fuse_workspace_bytes(2, 8, 300, 1000) == 2 * 4096 * 8 + 2 * 1000 * 40
    assert h.dy_tile_fuse_workspace_bytes(1, 109, 300, 4096) == 32768 * 8 + 4096 * 40
    assert h.dy_tile_fuse_workspace_bytes(1, 110, 300, 1000) == -1 and h.dy_tile_fuse_workspace_bytes(1, 8, 300, 4097) == -1
    assert h.dy_tile_fuse_workspace_bytes(0, 1, 1, 1) == -1 and h.dy_tile_fuse_workspace_bytes(1, 1, 1, 0) == -1


def test_tile_fuse_descriptor_mirror_matches_header():
    import subprocess
    import tempfile

    import drone_yolo_amd._lib as L

    fields = ("frames", "thr", "mode", "out", "out_members")
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "s.c")
        open(src, "w").write('#include <stdio.h>\n#include <stddef.h>\n#include "dyolo.h"\nint main(){printf("%zu' + " %zu" * len(fields) + '\\n", sizeof(dy_tile_fuse_desc)'
                             + "".join(f", offsetof(dy_tile_fuse_desc, {n})" for n in fields) + ");return 0;}\n")
        exe = os.path.join(td, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    D = L.TileFuseDesc
    assert got == [ctypes.sizeof(D)] + [getattr(D, n).offset for n in fields]


@functools.lru_cache(maxsize=None)
def _rows(name):
    F, K, md, nc, hw, tile, ov = CASES[name]
    return tile_rows(SEEDS[name], F, K, md, nc, hw, tile, ov, with_meta=True)


@pytest.mark.parametrize("name", ["one_tile", "lds", "4k"])
def test_fuse_ref_keeps_what_merge_ref_keeps(name):
    F, K, md, nc, hw = CASES[name][:5]
    rows, counts, offs = _rows(name)[:3]
    keep = 4096
    filled = absorbed = 0
    for metric, thr in ((0, IOU_THR), (1, IOS_THR)):
        for agnostic in (False, True):
            so, sc, si = merge_ref(rows, counts, offs, hw, thr, metric, agnostic, keep)
            uo, uc, ui, um = fuse_ref(rows, counts, offs, hw, thr, metric, agnostic, keep, "union")
            wo, wc, wi, wm = fuse_ref(rows, counts, offs, hw, thr, metric, agnostic, keep, "wbf")
            for o, c, i, m in ((uo, uc, ui, um), (wo, wc, wi, wm)):
                assert np.array_equal(c, sc) and np.array_equal(i, si)
                assert np.array_equal(o[..., 4:].view(np.uint32), so[..., 4:].view(np.uint32))  # conf and cls bit-equal
                assert m.dtype == np.int32 and np.array_equal(m, um)
                for f in range(F):
                    assert (m[f, : c[f]] >= 1).all() and not m[f, c[f] :].any() and not o[f, c[f] :].any()
                    if c[f] < keep:  # the scan reached every candidate: each is kept or absorbed
                        assert m[f].sum() == counts[f * K : (f + 1) * K].sum()
                    else:
                        filled += 1
            if name == "one_tile":
                continue
            one = um == 1
            assert one.any() and np.array_equal(wo[one].view(np.uint32), so[one].view(np.uint32))  # wbf rows with one member: merge_ref's, bit for bit
            assert np.array_equal(uo[one].view(np.uint32), so[one].view(np.uint32))
            many = um >= 2
            absorbed += int(many.sum())
            # every wbf box lies inside the union box of its row -- to the grid of the integer mean: a weighted mean of rint(coord * 64) / 64 lies
            # between the smallest and the largest of them, each within 1 / 128 of its coordinate, and is rounded to fp32 once (derived, not measured)
            q = np.float32(1 / 128) + np.spacing(np.float32(max(hw)))
            assert (wo[many, 0] >= uo[many, 0] - q).all() and (wo[many, 1] >= uo[many, 1] - q).all()
            assert (wo[many, 2] <= uo[many, 2] + q).all() and (wo[many, 3] <= uo[many, 3] + q).all()
            assert (uo[many, 0] <= so[many, 0]).all() and (uo[many, 2] >= so[many, 2]).all()  # and the union holds the row's own box
    if name == "4k":
        assert filled > 0  # merge_max_det = 4096 is reached: dropped rows are expected there
    if name != "one_tile":
        assert absorbed > 0


@pytest.mark.parametrize("name", ["lds", "4k"])
def test_fuse_ref_rows_behind_the_stop_are_absorbed_or_dropped(name):
    """At merge_max_det = 16 the scan stops early.  A candidate behind the stop is a member of the first kept row that matches it, and of none
    otherwise; a kept row's members at 16 are those it has without the stop (the first match of a candidate lies among the first 16 kept rows
    or not at all, and rows kept later only take candidates that none of the first 16 matches)."""
    F, K, md, nc, hw = CASES[name][:5]
    rows, counts, offs = _rows(name)[:3]
    full = fuse_ref(rows, counts, offs, hw, IOS_THR, 1, False, 4096, "union")
    cut = fuse_ref(rows, counts, offs, hw, IOS_THR, 1, False, 16, "union")
    cut_w = fuse_ref(rows, counts, offs, hw, IOS_THR, 1, False, 16, "wbf")
    dropped = 0
    for f in range(F):
        n = int(counts[f * K : (f + 1) * K].sum())
        c = int(cut[1][f])
        assert c == min(16, int(full[1][f])) and np.array_equal(cut[3][f], cut_w[3][f])
        assert np.array_equal(cut[2][f, :c], full[2][f, :c]) and np.array_equal(cut[3][f, :c], full[3][f, :c])
        assert np.array_equal(cut[0][f, :c].view(np.uint32), full[0][f, :c].view(np.uint32))
        dropped += n - int(cut[3][f].sum())
        assert c <= int(cut[3][f].sum()) <= n
    assert dropped > 0 and (cut[3] >= 2).any()


def test_union_restores_the_cut_objects_that_suppression_clips():
    """The point of the feature, on the generated rows (case lds, seed 1, IoS 0.8, class-aware): for every cut object whose views all survive,
    the union row spans the widest view of the object, while suppression keeps the clipped part where that scored higher."""
    F, K, md, nc, hw = CASES["lds"][:5]
    rows, counts, offs, obj, cuts, _ = _rows("lds")
    so, sc, si = merge_ref(rows, counts, offs, hw, IOS_THR, 1, False, 4096)
    uo, uc, ui, um = fuse_ref(rows, counts, offs, hw, IOS_THR, 1, False, 4096, "union")
    n_cut = n_clipped = 0
    for f in range(F):
        slots = si[f, : sc[f]]
        kept_obj = obj[f * K + slots // md, slots % md]
        for o in cuts[f]:
            t, r = np.nonzero(obj[f * K : (f + 1) * K] == o)
            x1 = rows[f * K + t, r, 0] + offs[t, 1].astype(np.float32)
            x2 = rows[f * K + t, r, 2] + offs[t, 1].astype(np.float32)
            widest = int(np.argmax(x2 - x1))
            (k,) = np.nonzero(kept_obj == o)[0]  # IoS keeps a cut object once
            assert um[f, k] == len(t)  # all its views are members of that row
            assert uo[f, k, 0] <= x1[widest] and uo[f, k, 2] >= x2[widest]
            n_cut += 1
            n_clipped += bool(so[f, k, 2] - so[f, k, 0] < 0.8 * (x2[widest] - x1[widest]))
    assert (n_cut, n_clipped) == (3, 2)  # of the three cut objects suppression returns the clipped part for two
    assert int((um - 1).clip(0).sum()) == 658 and int(um.max()) == 4  # rows absorbed over the frames; most members of one row


def test_split_object_no_tile_sees_whole():
    rows, counts, offs = split_rows()
    out, cnt, _ = merge_ref(rows, counts, offs, SPLIT_FRAME, 0.6, 0, False, 8)
    assert cnt[0] == 2  # IoU = 320 / 1080: both parts survive
    out, cnt, _ = merge_ref(rows, counts, offs, SPLIT_FRAME, 0.8, 1, False, 8)
    assert cnt[0] == 1 and out[0, 0].tolist() == [46.0, 10.0, 64.0, 30.0, np.float32(0.9), 1.0]  # IoS = 16 / 18: the fragment survives
    out, cnt, idx, mem = fuse_ref(rows, counts, offs, SPLIT_FRAME, 0.8, 1, False, 8, "union")
    assert cnt[0] == 1 and idx[0, 0] == 0 and mem[0].tolist() == [2] + [0] * 7
    assert out[0, 0].tolist() == [46.0, 10.0, 100.0, 30.0, np.float32(0.9), 1.0] and not out[0, 1:].any()
    out, cnt, idx, mem = fuse_ref(rows, counts, offs, SPLIT_FRAME, 0.8, 1, False, 8, "wbf")
    w0, w1 = round(0.9 * 65536), round(0.8 * 65536)  # the integer weights; x1 = (w0 * 46 + w1 * 48) / (w0 + w1)
    assert mem[0, 0] == 2 and out[0, 0, 0] == np.float32((w0 * 46 * 64 + w1 * 48 * 64) / (w0 + w1) / 64) and 64 < out[0, 0, 2] < 100


def test_predictor_refuses_bad_merge_mode_before_device_work():
    import drone_yolo_amd as D
    from drone_yolo_amd import hip_ops as H

    assert H.TILE_MERGE_MODES == {"suppress": 0, "union": 1, "wbf": 2}
    model = D.DetectionModel(dict(load_yaml("yolov8-p2-repvgg.yaml", "n", 10)), nc=10, verbose=False)
    P = D.engine.predictor.DetectionPredictor
    with pytest.raises(ValueError, match="merge_mode"):
        P(model, dict(tile=128, merge_mode="average", device="cpu"))
    for mode in ("union", "wbf", "suppress", "Union"):  # accepted: construction gets past every tile check, to the device selection (none here)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            P(model, dict(tile=128, merge_mode=mode, device="cpu"))
    import yaml

    assert yaml.safe_load(open(os.path.join(ROOT, "drone-yolo_amd", "cfg", "default.yaml")))["merge_mode"] == "suppress"
