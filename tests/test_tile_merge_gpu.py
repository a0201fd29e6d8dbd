"""GPU: the batched tile slicer and the one-launch cross-tile merge (csrc/tile_merge.hip) against the numpy restatement of
tests/_tile_util.py, the parent chain (dy_rows_to_pred -> dy_nms) and the single-frame slicer; then ``tile=`` through YOLO.predict /
YOLO.track against the CPU oracle chain with the merge done by ``merge_ref``."""
import functools
import types

import numpy as np
import pytest
import torch

import drone_yolo_amd as D
from drone_yolo_amd import hip_ops as H
from drone_yolo_amd._lib import lib
from oracle import drone_yolo_oracle as O
from tests._tile_util import CASES, IOS_THR, IOU_THR, MARGIN, SEEDS, block_frame, merge_margin, merge_ref, oracle_tile_chain, tile_rows
from tests._track_util import assert_rows_match
from tests._util import golden
from tests.test_model_gpu import _build

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _rows(name):
    return tile_rows(SEEDS[name], *CASES[name])


@functools.lru_cache(maxsize=None)
def _ref(name, metric, agnostic, keep):
    rows, counts, offs = _rows(name)
    return merge_ref(rows, counts, offs, CASES[name][4], IOS_THR if metric else IOU_THR, metric, agnostic, keep)


def _device_rows(name, device):
    rows, counts, offs = _rows(name)
    return torch.from_numpy(rows).to(device), torch.from_numpy(counts).to(device), torch.from_numpy(offs).to(device)


# ---- dy_tile_merge against merge_ref --------------------------------------------------------------------------------------------------
# (case, merge_max_det): one tile; the LDS sort with ragged counts and an empty frame; the same truncated in the middle of a chunk of 64;
# 12,000 slots (at 4096 kept rows the kept list leaves LDS for 4096 keys: the workspace sort); 32,700 slots, sorted in the workspace
MERGE_RUNS = [("one_tile", 1000), ("lds", 1000), ("lds", 16), ("4k", 1000), ("4k", 4096), ("limit", 1000), ("limit", 4096)]


@pytest.mark.parametrize("agnostic", [False, True], ids=["by_class", "agnostic"])
@pytest.mark.parametrize("metric", [0, 1], ids=["iou", "ios"])
@pytest.mark.parametrize("name,keep", MERGE_RUNS, ids=[f"{n}-{k}" for n, k in MERGE_RUNS])
def test_tile_merge_matches_numpy_restatement(device, name, keep, metric, agnostic):
    F, K, md, nc, hw = CASES[name][:5]
    rows, counts, offs = _device_rows(name, device)
    got = H.tile_merge((rows, counts), offs, K, hw, nc, IOS_THR if metric else IOU_THR, metric, agnostic, keep)
    out, cnt, idx = got.out.cpu().numpy(), got.count.cpu().numpy(), got.index.cpu().numpy()
    eo, ec, ei = _ref(name, metric, agnostic, keep)
    assert (got.batch, got.max_det) == (F, keep) and out.shape == (F, keep, 6) and idx.shape == (F, keep)
    assert np.array_equal(cnt, ec), (cnt, ec)
    assert np.array_equal(idx, ei)  # the same slots in the same order, -1 beyond the count
    assert np.array_equal(out.view(np.uint32), eo.view(np.uint32))  # rows bit-equal, rows >= count zero
    if name == "lds":
        assert cnt[1] == 0 and (cnt[[0, 2]] == keep if keep == 16 else cnt[[0, 2]] > 16).all()  # a frame with no rows; truncation mid-chunk at 16


def test_tile_merge_metrics_differ_where_they_should(device):
    """On the generated rows the IoS merge keeps fewer boxes than the IoU merge (the cut objects), and an agnostic merge fewer than a
    class-aware one (views whose class the generator flipped): the flags reach the kernel."""
    F, K, md, nc, hw = CASES["lds"][:5]
    rows, counts, offs = _device_rows("lds", device)
    n = {}
    for metric in (0, 1):
        for agnostic in (False, True):
            n[metric, agnostic] = H.tile_merge((rows, counts), offs, K, hw, nc, IOS_THR if metric else IOU_THR, metric, agnostic, 4096).count.cpu().numpy().copy()
    assert (n[1, False][[0, 2]] < n[0, False][[0, 2]]).all() and (n[0, True][[0, 2]] < n[0, False][[0, 2]]).all() and (n[1, True][[0, 2]] < n[1, False][[0, 2]]).all()


# ---- dy_tile_merge (IoU) against the parent chain: dy_rows_to_pred -> dy_nms(conf 0) on the same rows, one frame at a time ----------------
@pytest.mark.parametrize("name,keep", [("parent6", 1000), ("parent40", 1000)])  # (at 12,000 anchors the parent's kernel has no LDS for a longer kept list)
def test_tile_merge_iou_keeps_what_the_parent_chain_keeps(device, name, keep):
    F, K, md, nc, hw = CASES[name][:5]
    assert F == 1
    rows, counts, offs = _device_rows(name, device)
    pred = torch.empty((1, 4 + nc, K * md), dtype=torch.float32, device=device)
    H.check(lib().dy_rows_to_pred(rows.data_ptr(), counts.data_ptr(), offs.data_ptr(), pred.data_ptr(), K, md, nc, torch.cuda.current_stream().cuda_stream))
    parent = H.nms(pred, 0.0, IOU_THR, max_det=keep, nc=nc)
    pn = int(parent.count[0])
    pout, pidx = parent.out[0, :pn].cpu().numpy(), parent.index[0, :pn].cpu().numpy()
    got = H.tile_merge((rows, counts), offs, K, hw, nc, IOU_THR, 0, False, keep)
    n = int(got.count[0])
    out, idx = got.out[0, :n].cpu().numpy(), got.index[0, :n].cpu().numpy()
    assert n == pn and 0 < n < int(counts.sum()) and np.array_equal(idx, pidx)  # the same slots in the same order
    assert np.array_equal(out[:, 4:].view(np.uint32), pout[:, 4:].view(np.uint32))  # scores and classes bit-equal
    # the parent's centre / size round trip, (x1 + x2) / 2 -+ (x2 - x1) / 2, rounds twice at the magnitude of the coordinate (once more at twice it):
    # within 4 ulp of the frame's largest coordinate.  Derived, not measured.
    tol = 4 * float(np.spacing(np.float32(max(hw))))
    err = np.abs(out[:, :4].astype(np.float64) - pout[:, :4].astype(np.float64)).max()
    assert err <= tol, (err, tol)


# ---- the batched slicer against the single-frame slicer ---------------------------------------------------------------------------------
@pytest.mark.parametrize("swap_rb", [0, 1])
@pytest.mark.parametrize("tile", [128, 126], ids=["float4", "scalar"])  # 126: a tile width that is no multiple of four takes the scalar stores
def test_tiles_batch_is_bit_equal_to_single_frame_slicer(device, swap_rb, tile):
    hf, wf = 200, 301  # a width that is no multiple of 4
    frames = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (3, hf, wf, 3), dtype=np.uint8)).to(device)
    offs = torch.tensor([(0, 0), (72, 173), (100, 200), (150, 250), (190, 299), (31, 86)], dtype=torch.int32, device=device)  # overhanging right and bottom
    k, st = len(offs), torch.cuda.current_stream().cuda_stream
    single = torch.empty((3, k, 3, tile, tile), dtype=torch.float32, device=device)
    for f in range(3):
        H.check(lib().dy_tiles_u8_to_nchw_f32(frames[f].data_ptr(), offs.data_ptr(), single[f].data_ptr(), k, hf, wf, tile, tile, swap_rb, 114.0, st))
    one = H.tiles_batch(frames[:1].contiguous(), offs, tile, swap_rb=bool(swap_rb))
    assert one.shape == (k, 3, tile, tile) and torch.equal(one, single[0])
    three = torch.full((3 * k, 3, tile, tile), -1.0, dtype=torch.float32, device=device)
    assert H.tiles_batch(frames, offs, tile, out=three, swap_rb=bool(swap_rb)) is three
    assert torch.equal(three.view(3, k, 3, tile, tile), single)
    assert float(three[4, :, 64:, 64:].max()) == pytest.approx(114.0 / 255.0)  # tile 4 starts at the last row / column: all padding beyond


# ---- tile= through the public interface ------------------------------------------------------------------------------------------------
TILE, OVERLAP, MERGE = 128, 0.25, 0.6
ARGS = dict(tile=TILE, tile_overlap=OVERLAP, merge_iou=MERGE, dtype="fp32", device=0)
# block_frame seeds, chosen on the CPU oracle (see _expected): 200 x 300 frames whose merge removes cross-tile duplicates; 100 x 90 frames (smaller
# than the tile); 200 x 300 frames on which the IoS merge drops boxes the IoU merge keeps (a box cut at a tile border beside the whole box)
FRAME_SEEDS = (4, 7, 13, 50, 70)
SMALL_SEEDS = (2, 6)
IOS_SEEDS = (4, 7)
SCORE_MARGIN = 1e-4


@pytest.fixture(scope="module")
def chain(device):
    """The fixture model behind YOLO and, per frame, the CPU oracle's per-tile rows (computed once, shared, not modified)."""
    m, d, sd, model, _ = _build("n128", golden("e2e.npz"), device)
    yolo = D.YOLO(m["yaml"])
    yolo.model = model
    nc = m["nc"]

    @functools.lru_cache(maxsize=None)
    def oracle(seed, shape):
        frame = block_frame(seed, shape)
        rows, counts, offs, margins = oracle_tile_chain(O, d, sd, frame, TILE, OVERLAP, nc)
        return frame, rows, counts, offs, margins

    return types.SimpleNamespace(yolo=yolo, nc=nc, oracle=oracle)


def _expected(chain, seed, shape, metric=0):
    """The oracle's rows of one frame, merged by merge_ref, after asserting that the oracle keeps clear of every threshold of the chain, so that
    the device's fp32 round-off cannot change a decision: same-class IoUs among a tile's candidates >= 0.02 from the NMS threshold 0.7, same-class
    overlaps among the per-tile rows >= 0.02 from the merge threshold 0.6, and EVERY anchor's best class score (kept or not) >= 1e-4 from conf 0.25.
    The score margin asked for at first, 5e-3 on the kept rows, no frame can meet with this fixture: the model's class scores all lie in
    [0.21, 0.27] and the zero padding at a tile's corners alone gives every tile a row at 0.2509 (a flat grey frame: margin 0.0009; none of 600
    seeded frames of four kinds reached 5e-3).  1e-4 is what fp32 allows to ask: a score is a sigmoid (slope <= 1/4) of a logit accumulated in
    fp32 over ~25 layers of <= 576 products, ~1e-5 of round-off at worst, and it is asked of all 8,160 anchors on both sides of conf."""
    frame, rows, counts, offs, (m_conf, m_nms) = chain.oracle(seed, shape)
    assert counts.sum() > 0 and m_conf >= SCORE_MARGIN, f"frame {seed}: an anchor's score within {SCORE_MARGIN} of conf ({m_conf})"
    assert m_nms >= MARGIN, f"frame {seed}: a same-class IoU within {MARGIN} of the per-tile NMS threshold"
    assert merge_margin(rows, counts, offs, MERGE, metric) >= MARGIN, f"frame {seed}: a same-class overlap within {MARGIN} of the merge threshold"
    out, cnt, _ = merge_ref(rows, counts, offs, shape, MERGE, metric, False, 1000)
    return frame, out[0, : cnt[0]], int(counts.sum())


def _assert_result(res, frame, exp, shape, what, same_object=True):
    got = res.boxes.data.cpu().numpy()
    assert res.orig_shape == tuple(shape) and (res.orig_img is frame if same_object else np.array_equal(res.orig_img, frame)), what
    assert got.shape == exp.shape, f"{what}: {got.shape[0]} rows, expected {exp.shape[0]}"
    assert np.array_equal(got[:, 5], exp[:, 5]), f"{what}: classes differ"
    assert np.allclose(got[:, :5], exp[:, :5], atol=3e-2, rtol=1e-4), f"{what}: boxes / scores differ by {np.abs(got[:, :5] - exp[:, :5]).max()}"


def test_predict_tile_matches_oracle_chain(chain):
    shape = (200, 300)
    exp = [_expected(chain, s, shape) for s in FRAME_SEEDS[:3]]
    res = chain.yolo.predict([e[0] for e in exp], **ARGS)
    assert isinstance(res, list) and len(res) == 3
    for i, (frame, rows, n_tile_rows) in enumerate(exp):
        assert 0 < len(rows) < n_tile_rows  # the merge removed cross-tile duplicates
        _assert_result(res[i], frame, rows, shape, f"frame {i}")


def test_predict_tile_one_call_batches_and_stream_agree(chain):
    shape = (200, 300)
    exp = [_expected(chain, s, shape) for s in FRAME_SEEDS]
    frames = [e[0] for e in exp]
    streamed = chain.yolo.predict(frames, batch=2, stream=True, **ARGS)
    assert isinstance(streamed, types.GeneratorType)
    for what, res in (("one call", chain.yolo.predict(frames, **ARGS)), ("batch=2", chain.yolo.predict(frames, batch=2, **ARGS)), ("stream", list(streamed))):
        assert len(res) == len(frames)
        for i, (frame, rows, _) in enumerate(exp):
            _assert_result(res[i], frame, rows, shape, f"{what}, frame {i}")
    as_tensor = chain.yolo.predict(torch.from_numpy(np.stack(frames)), batch=3, **ARGS)  # a uint8 (N, H, W, 3) tensor is the same source
    for i, (frame, rows, _) in enumerate(exp):
        _assert_result(as_tensor[i], frame, rows, shape, f"tensor source, frame {i}", same_object=False)


def test_predict_tile_mixed_shapes_keep_source_order(chain):
    big, small = (200, 300), (100, 90)  # 100 x 90 is smaller than the tile: one tile padded with 114
    plan = [(FRAME_SEEDS[0], big), (SMALL_SEEDS[0], small), (FRAME_SEEDS[1], big), (SMALL_SEEDS[1], small)]
    exp = [_expected(chain, s, sh) for s, sh in plan]
    res = chain.yolo.predict([e[0] for e in exp], **ARGS)
    assert len(res) == len(plan)
    for i, ((frame, rows, _), (_, sh)) in enumerate(zip(exp, plan)):
        _assert_result(res[i], frame, rows, sh, f"mixed, frame {i}")
        alone = chain.yolo.predict([frame], **ARGS)[0]
        assert alone.orig_shape == sh and np.array_equal(res[i].boxes.data.cpu().numpy(), alone.boxes.data.cpu().numpy())


def test_predict_tile_ios_merges_border_cut_boxes(chain):
    shape = (200, 300)
    iou = [_expected(chain, s, shape, 0) for s in IOS_SEEDS]
    ios = [_expected(chain, s, shape, 1) for s in IOS_SEEDS]
    frames = [e[0] for e in iou]
    res_iou = chain.yolo.predict(frames, **ARGS)
    res_ios = chain.yolo.predict(frames, merge_metric="ios", **ARGS)
    for i in range(len(frames)):
        assert len(ios[i][1]) < len(iou[i][1]) and len(res_ios[i]) < len(res_iou[i])
        _assert_result(res_iou[i], frames[i], iou[i][1], shape, f"iou, frame {i}")
        _assert_result(res_ios[i], frames[i], ios[i][1], shape, f"ios, frame {i}")


def test_predict_tile_refuses_float_tensors_and_untrackable_sizes(chain):
    with pytest.raises(NotImplementedError, match="cut from pixels"):
        chain.yolo.predict(torch.rand(1, 3, 128, 128), **ARGS)
    with pytest.raises(ValueError, match="1024"):
        chain.yolo.track([block_frame(0, (200, 300))], merge_max_det=1025, **ARGS)


def test_track_tile_device_tracker_equals_host_tracker(chain):
    """The same merged rows through the track step on the device and through the host tracker; persist=True goes on across two calls."""
    base = block_frame(FRAME_SEEDS[0], (200, 300))
    frames = [np.ascontiguousarray(np.roll(base, (2 * f, 3 * f), (0, 1))) for f in range(6)]  # a short video: the frame drifting a few pixels per step
    targs = dict(conf=0.25, **ARGS)
    dev = chain.yolo.track(frames, batch=3, **targs)
    dev_a = chain.yolo.track(frames[:3], **targs)
    dev_b = chain.yolo.track(frames[3:], persist=True, **targs)
    host = chain.yolo.track(frames, batch=3, device_track=False, **targs)
    host_a = chain.yolo.track(frames[:3], device_track=False, **targs)
    host_b = chain.yolo.track(frames[3:], persist=True, device_track=False, **targs)
    assert len(dev) == len(host) == 6 and any(r.boxes.is_track for r in dev)
    det = chain.yolo.predict(frames, conf=0.25, **ARGS)
    for f in range(6):
        assert dev[f].orig_shape == (200, 300) and dev[f].orig_img is frames[f]
        assert dev[f].boxes.is_track == host[f].boxes.is_track
        if dev[f].boxes.is_track:
            assert_rows_match(dev[f].boxes.data.cpu().numpy(), host[f].boxes.data.cpu().numpy(), f"frame {f}")
            assert len(dev[f]) <= len(det[f])  # tracks are made of the frame's merged rows
    for f, (d2, h2) in enumerate(zip(dev_a + dev_b, host_a + host_b)):
        assert d2.boxes.is_track == h2.boxes.is_track
        if d2.boxes.is_track:
            assert_rows_match(d2.boxes.data.cpu().numpy(), h2.boxes.data.cpu().numpy(), f"persist, frame {f}")
            assert np.array_equal(d2.boxes.data.cpu().numpy(), dev[f].boxes.data.cpu().numpy())  # two calls with persist = one call
