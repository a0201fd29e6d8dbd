"""GPU: the one-launch cross-tile merge for oriented boxes (``dy_tile_merge_rotated``, csrc/tile_merge.hip) against the numpy restatement of
tests/_tile_rot_util.py, and ``tile=`` through ``YOLO.predict`` on an ``-obb`` model.

Kernel: counts and ``index`` equal, rows bit-equal (outputs are copies, one exact add and clamps), rows past the count zero -- on inputs that
keep the margin tests/test_tile_merge_rotated_host.py asserts, so the device's own sinf / cosf / logf / expf cannot change a verdict.
End to end: the ``Results.obb.data`` of a tiled predict equal the restatement applied to the per-tile rows the pass itself produced (read
from the predictor's compiled forward; the margin is asserted on them first), and those per-tile rows are what an ordinary predict of each
tile crop returns."""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

from drone_yolo_amd import _lib
from drone_yolo_amd import hip_ops as H
from tests import _tile_rot_util as T
from tests._fuse_util import fuse_ref
from tests._tile_util import IOU_THR, block_frame, merge_ref
from tests._util import golden
from tests.test_obb_gpu import _yolo

pytestmark = pytest.mark.gpu


def _dev(arrays, device):
    return tuple(torch.from_numpy(np.array(a)).to(device) for a in arrays)  # (a copy: the shared arrays are read-only)


def _assert_equal(got, ref, keep, what):
    eo, ec, ei = ref
    out, cnt, idx = got.out.cpu().numpy(), got.count.cpu().numpy(), got.index.cpu().numpy()
    assert out.shape == eo.shape and idx.shape == ei.shape and got.max_det == keep, what
    assert np.array_equal(cnt, ec), f"{what}: kept {cnt.tolist()}, the restatement {ec.tolist()}"
    assert np.array_equal(idx, ei), f"{what}: other slots than the restatement"  # the same slots in the same order, -1 beyond the count
    assert np.array_equal(out.view(np.uint32), eo.view(np.uint32)), f"{what}: rows differ"  # bit-equal, rows >= count zero


# ---- dy_tile_merge_rotated against merge_ref_rotated -----------------------------------------------------------------------------------
@pytest.mark.parametrize("agnostic", [False, True], ids=["by_class", "agnostic"])
@pytest.mark.parametrize("name,keep", T.RUNS, ids=[f"{n}-{k}" for n, k in T.RUNS])
def test_tile_merge_rotated_matches_numpy_restatement(device, name, keep, agnostic):
    F, K, md, nc, hw = T.CASES[name][:5]
    rows, counts, offs = _dev(T.case_rows(name), device)
    got = H.tile_merge_rotated((rows, counts), offs, K, hw, nc, T.THR, agnostic, keep)
    assert isinstance(got, H.RTileMergeBuffers) and (got.batch, got.ROW) == (F, 7)
    _assert_equal(got, T.case_ref(name, agnostic, keep), keep, f"{name} keep {keep}")


@pytest.mark.parametrize("name", T.HAND_CASES)
def test_tile_merge_rotated_hand_cases(device, name):
    """chain: greedy keeps A and C; same place, two classes; (ox, oy) the right way round; clamps; degenerate rows alone in their classes."""
    rows, counts, offs, expect = T.hand_case(name)
    d = _dev((rows, counts, offs), device)
    for agnostic, slots in expect.items():
        got = H.tile_merge_rotated(d[:2], d[2], len(offs), T.HAND_FRAME, 3, T.THR, agnostic, 16)
        _assert_equal(got, T.merge_ref_rotated(rows, counts, offs, T.HAND_FRAME, T.THR, agnostic, 16), 16, f"{name} agnostic {agnostic}")
        assert got.index[0, : len(slots)].tolist() == slots and int(got.count[0]) == len(slots)


def test_tile_merge_rotated_entry_point_refuses_before_any_launch(device):
    h = _lib.lib()
    rows, counts, offs = _dev(T.case_rows("one_tile"), device)
    bufs = H.RTileMergeBuffers(1, 1, 300, 1000, device)

    def desc(**kw):
        d = _lib.TileMergeRotatedDesc()
        d.rows, d.counts, d.offsets_yx = rows.data_ptr(), counts.data_ptr(), offs.data_ptr()
        d.frames, d.tiles, d.max_det, d.nc, d.frame_h, d.frame_w = 1, 1, 300, 3, 64, 64
        d.thr, d.agnostic, d.merge_max_det = T.THR, 0, 1000
        d.out, d.out_count, d.out_index = bufs.out.data_ptr(), bufs.count.data_ptr(), bufs.index.data_ptr()
        d.workspace, d.workspace_bytes = bufs.workspace.data_ptr(), bufs.workspace.numel()
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    call = lambda d: h.dy_tile_merge_rotated(ctypes.byref(d), None)  # noqa: E731
    before = (bufs.out.clone().fill_(7), bufs.count.clone().fill_(7))
    bufs.out.fill_(7), bufs.count.fill_(7)
    assert call(desc(tiles=32769, max_det=1)) == -2 and b"32768" in h.dy_last_error_string()  # DY_ERR_UNSUPPORTED
    assert call(desc(merge_max_det=4097)) == -2 and b"4096" in h.dy_last_error_string()
    assert call(desc(workspace_bytes=bufs.workspace.numel() - 8)) == -4  # DY_ERR_WORKSPACE
    assert call(desc(rows=None)) == -1 and call(desc(out_count=None)) == -1 and call(desc(workspace=None)) == -1  # DY_ERR_INVALID_ARG
    assert call(desc(thr=1.5)) == -1 and call(desc(frame_w=0)) == -1
    assert h.dy_tile_merge_rotated(None, None) == -1
    assert h.dy_tile_merge_rotated_workspace_bytes(1, 32769, 1) == -1 and h.dy_tile_merge_rotated_workspace_bytes(2, 40, 300) == 2 * 16384 * 8
    torch.cuda.synchronize(device)
    assert torch.equal(bufs.out, before[0]) and torch.equal(bufs.count, before[1]), "a refused call must not launch"
    assert call(desc(out_index=None)) == 0  # the index is optional
    torch.cuda.synchronize(device)
    assert int(bufs.count[0]) == int(T.case_ref("one_tile", False, 1000)[1][0])
    with pytest.raises(ValueError, match="7"):
        H.tile_merge_rotated((rows[:, :, :6].contiguous(), counts), offs, 1, (64, 64), 3, T.THR)
    with pytest.raises(ValueError, match="32768"):
        H.RTileMergeBuffers(1, 110, 300, 1000, device)


def test_tile_merge_rotated_is_deterministic_and_leaves_no_stale_rows(device):
    F, K, md, nc, hw = T.CASES["ragged"][:5]
    rows, counts, offs = _dev(T.case_rows("ragged"), device)
    a = H.RTileMergeBuffers(F, K, md, 1000, device)
    b = H.RTileMergeBuffers(F, K, md, 1000, device)
    for bufs in (a, b):
        bufs.out.fill_(float("nan")), bufs.index.fill_(12345), bufs.count.fill_(-9)
        assert H.tile_merge_rotated((rows, counts), offs, K, hw, nc, T.THR, False, 1000, bufs=bufs) is bufs
    assert torch.equal(a.out.view(torch.int32), b.out.view(torch.int32)) and torch.equal(a.index, b.index) and torch.equal(a.count, b.count)
    # the same buffers behind a smaller input: frame 0 has no rows any more, frame 2 at most five per tile
    fewer = counts.clone()
    fewer[:K] = 0
    fewer[K:] = torch.clamp(fewer[K:], max=5)
    host_rows, _, host_offs = T.case_rows("ragged")
    _, p64, p32 = T.greedy64(host_rows, fewer.cpu().numpy(), host_offs, T.THR, False, 1000)
    m, dist = T.margin(p64, p32, T.THR)
    assert dist >= m
    assert int(a.count[0]) > 0
    H.tile_merge_rotated((rows, fewer), offs, K, hw, nc, T.THR, False, 1000, bufs=a)
    _assert_equal(a, T.merge_ref_rotated(host_rows, fewer.cpu().numpy(), host_offs, hw, T.THR, False, 1000), 1000, "reused buffers")
    assert int(a.count[0]) == 0 and not bool(a.out[0].any()) and bool((a.index[0] == -1).all()) and 0 < int(a.count[2]) <= 5 * K


def test_one_buffer_cache_keeps_the_three_merges_apart(device):
    """``tile_merge``, ``tile_merge_rotated`` and ``tile_merge(mode="union")`` at one (F, K, max_det, merge_max_det) = (1, 1, 8, 16), forwards and
    backwards: the cache they share hands each its own class of buffers (6 / 7 / 6 floats a row), the same object to a repeated call, and every
    result is its restatement's -- the suppressing call's also once ``members`` exists.  Three rows per kind: two of one class that overlap above
    the threshold (IoU 380 / 420 against 0.6; views of one oriented box half a pixel apart) and one far from both."""
    hw, K, md, keep, nc = (64, 64), 1, 8, 16, 3
    axis, rot = np.zeros((1, md, 6), np.float32), np.zeros((1, md, 7), np.float32)
    axis[0, :3] = [[10, 10, 30, 30, 0.9, 1], [11, 10, 31, 30, 0.8, 1], [40, 40, 60, 60, 0.7, 1]]
    rot[0, :3] = [[20, 20, 20, 10, 0.3, 0.9, 1], [20.5, 20.25, 20, 10, 0.3, 0.8, 1], [48, 48, 20, 10, 0.3, 0.7, 1]]
    counts, offs = np.array([3], np.int32), np.zeros((1, 2), np.int32)
    kept, p64, p32 = T.greedy64(rot, counts, offs, T.THR, False, keep)
    m, dist = T.margin(p64, p32, T.THR)
    assert len(p64) == 2 and kept[0].tolist() == [0, 2] and dist >= m, (p64, m, dist)  # both decided pairs keep the margin from the threshold
    exp = {"suppress": merge_ref(axis, counts, offs, hw, IOU_THR, 0, False, keep), "union": fuse_ref(axis, counts, offs, hw, IOU_THR, 0, False, keep, "union"),
           "rotated": T.merge_ref_rotated(rot, counts, offs, hw, T.THR, False, keep)}
    assert all(e[1][0] == 2 and e[2][0, :2].tolist() == [0, 2] for e in exp.values()) and exp["union"][3][0, :3].tolist() == [2, 1, 0]
    da, dr, dc, do = _dev((axis, rot, counts, offs), device)
    calls = {"suppress": lambda: H.tile_merge((da, dc), do, K, hw, nc, IOU_THR, 0, False, keep),
             "rotated": lambda: H.tile_merge_rotated((dr, dc), do, K, hw, nc, T.THR, False, keep),
             "union": lambda: H.tile_merge((da, dc), do, K, hw, nc, IOU_THR, 0, False, keep, mode="union")}
    seen = {}
    for kind in ("suppress", "rotated", "union", "union", "rotated", "suppress"):
        got = calls[kind]()
        cls, row = (H.RTileMergeBuffers, 7) if kind == "rotated" else (H.TileMergeBuffers, 6)
        assert type(got) is cls and got.out.shape == (1, keep, row), kind
        assert seen.setdefault(kind, got) is got, f"{kind}: a repeated call returned other buffers"
        _assert_equal(got, exp[kind][:3], keep, kind)
        if kind == "union":
            assert np.array_equal(got.members.cpu().numpy(), exp[kind][3])
    assert seen["rotated"] is not seen["suppress"] and seen["rotated"] is not seen["union"]
    assert seen["suppress"].members is not None and seen["rotated"].members is None


# ---- tile= through YOLO.predict on an -obb model -----------------------------------------------------------------------------------------
TILE, OVERLAP, MERGE = 128, 0.25, 0.45
SHAPE, SMALL = (200, 300), (100, 90)  # 100 x 90 is smaller than the tile: one tile padded with 114
# block_frame seeds, found on the GPU among 0..39 (0..11 for the small frames): every one of those keeps the margin from MERGE in both
# precisions; these lose rows in the merge (18: 10 tile rows -> 5, 35: 7 -> 3, 38: 6 -> 2, 22: 5 -> 2; the small frames 2 -> 1)
FRAME_SEEDS = (18, 35, 38, 22, 0)
SMALL_SEEDS = (0, 3)
DTYPES = [("fp32", "f32"), (None, "split")]


@pytest.fixture(scope="module", params=DTYPES, ids=[d[1] for d in DTYPES])
def tiled(request, device):
    """The fixture OBB model behind YOLO and, per (seeds, shape), one tiled predict with the per-tile rows the pass produced and the
    restatement's merge of them (computed once, shared, not modified)."""
    g = golden("obb.npz")
    y, m = _yolo(g, "obbn64x96")
    args = dict(tile=TILE, tile_overlap=OVERLAP, merge_iou=MERGE, dtype=request.param[0], device=0, conf=m["conf"], iou=m["iou"])

    @functools.lru_cache(maxsize=None)
    def run(seeds, shape):
        frames = [block_frame(s, shape) for s in seeds]
        res = y.predict(frames, **args)
        p = y.predictor
        assert type(p).__name__ == "OBBPredictor"
        offs = np.asarray(T.tile_offsets(shape[0], shape[1], TILE, OVERLAP), np.int32)
        cf = p._compiled[((len(frames) * len(offs), 3, TILE, TILE), p.dtype)]
        rows, counts = cf.nms.out.cpu().numpy().copy(), cf.nms.count.cpu().numpy().copy()
        kept, p64, p32 = T.greedy64(rows, counts, offs, MERGE, False, 1000)
        margin, dist = T.margin(p64, p32, MERGE)
        print(f"{request.param[1]} seeds {seeds} {shape}: tile rows {counts.reshape(len(frames), -1).sum(1).tolist()}, kept {[len(k) for k in kept]}, "
              f"{len(p64)} pairs, M = {margin:.3e}, nearest pair {dist:.3e}")
        assert dist >= margin, f"frames {seeds}: a pair of per-tile rows lies {dist} from the merge threshold, the margin is {margin}"
        out, cnt, _ = T.merge_ref_rotated(rows, counts, offs, shape, MERGE, False, 1000)
        return frames, res, [out[f, : cnt[f]] for f in range(len(frames))], rows, counts, offs

    return types.SimpleNamespace(yolo=y, args=args, run=run, nc=m["nc"])


def _same(res, frame, exp, shape, what, exact=False, same_object=True):
    assert res.boxes is None and res.obb is not None and res.obb.data.is_cuda and res.orig_shape == tuple(shape), what
    assert res.orig_img is frame if same_object else np.array_equal(res.orig_img, frame), what
    got = res.obb.data.cpu().numpy()
    assert got.shape == exp.shape, f"{what}: {got.shape[0]} rows, expected {exp.shape[0]}"
    assert tuple(res.obb.xyxyxyxy.shape) == (len(exp), 4, 2)
    if exact:
        assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), f"{what}: rows are not the restatement's"
    else:  # another batch size records another pass: tests/test_tile_merge_gpu.py::_assert_result's allclose
        assert np.array_equal(got[:, 6], exp[:, 6]), f"{what}: classes differ"
        assert np.allclose(got[:, :6], exp[:, :6], atol=3e-2, rtol=1e-4), f"{what}: rows differ by {np.abs(got[:, :6] - exp[:, :6]).max()}"


def test_predict_tile_obb_is_the_restatement_on_the_rows_of_the_pass(tiled):
    frames, res, exp, rows, counts, offs = tiled.run(FRAME_SEEDS[:3], SHAPE)
    assert isinstance(res, list) and len(res) == 3
    per_frame = counts.reshape(3, -1).sum(1)
    for i in range(3):
        _same(res[i], frames[i], exp[i], SHAPE, f"frame {i}", exact=True)
    assert any(0 < len(exp[i]) < per_frame[i] for i in range(3)), "no frame loses cross-tile duplicates"


def test_predict_tile_obb_rows_are_those_of_each_crop_predicted_alone(tiled):
    frames, _, _, rows, counts, offs = tiled.run(FRAME_SEEDS[:3], SHAPE)
    crops = []
    for frame in frames:
        for oy, ox in offs:
            c = np.full((TILE, TILE, 3), 114, np.uint8)
            part = frame[oy : oy + TILE, ox : ox + TILE]
            c[: part.shape[0], : part.shape[1]] = part
            crops.append(torch.from_numpy(np.ascontiguousarray(c[:, :, ::-1].transpose(2, 0, 1))).float() / 255)
    plain = {k: v for k, v in tiled.args.items() if k not in ("tile", "tile_overlap", "merge_iou")}
    alone = tiled.yolo.predict(torch.stack(crops), **plain)
    assert len(alone) == len(counts)
    for t, r in enumerate(alone):
        got, exp = r.obb.data.cpu().numpy(), rows[t, : counts[t]]
        assert len(got) == counts[t] and np.array_equal(got[:, 6], exp[:, 6]), f"tile {t}: counts or classes differ"
        assert np.allclose(got[:, :6], exp[:, :6], atol=3e-2, rtol=1e-4), f"tile {t}: rows differ by {np.abs(got[:, :6] - exp[:, :6]).max(initial=0)}"


def test_predict_tile_obb_one_call_batches_stream_and_tensor_agree(tiled):
    frames, _, exp, _, _, _ = tiled.run(FRAME_SEEDS, SHAPE)
    streamed = tiled.yolo.predict(frames, batch=2, stream=True, **tiled.args)
    assert isinstance(streamed, types.GeneratorType)
    for what, res in (("one call", tiled.yolo.predict(frames, **tiled.args)), ("batch=2", tiled.yolo.predict(frames, batch=2, **tiled.args)), ("stream", list(streamed))):
        assert len(res) == len(frames)
        for i in range(len(frames)):
            _same(res[i], frames[i], exp[i], SHAPE, f"{what}, frame {i}")
    as_tensor = tiled.yolo.predict(torch.from_numpy(np.stack(frames)), batch=3, **tiled.args)  # a uint8 (N, H, W, 3) tensor is the same source
    for i in range(len(frames)):
        _same(as_tensor[i], frames[i], exp[i], SHAPE, f"tensor source, frame {i}", same_object=False)


def test_predict_tile_obb_mixed_shapes_keep_source_order(tiled):
    big = tiled.run(FRAME_SEEDS[:2], SHAPE)
    small = tiled.run(SMALL_SEEDS, SMALL)
    assert len(small[5]) == 1  # one tile
    plan = [(big, 0, SHAPE), (small, 0, SMALL), (big, 1, SHAPE), (small, 1, SMALL)]
    res = tiled.yolo.predict([r[0][i] for r, i, _ in plan], **tiled.args)
    assert len(res) == len(plan)
    for j, (r, i, shape) in enumerate(plan):
        _same(res[j], r[0][i], r[2][i], shape, f"mixed, frame {j}")
