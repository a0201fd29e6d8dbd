"""GPU: YOLO.track end to end on an oriented-box model -- the fixture OBB model of tests/golden/obb.npz behind YOLO as tests/test_obb_gpu.py
builds it, a short "video" made by shifting the fixture's uint8 frame a few pixels per frame, the rotated tracker behind dy_nms_rotated on
the device and on the host, persist / reset, streamed batches, two streams, frames without detections, predict afterwards."""
import numpy as np
import pytest
import torch

from tests._track_obb_util import assert_rows_match, margin_all, same_bits, sequences
from tests._util import golden
from tests.test_obb_gpu import _yolo

pytestmark = pytest.mark.gpu
TAG, SHIFT, FRAMES = "obbn_u8", (1, 2), 8  # fixture, (rows, columns) shifted per frame
M = margin_all(sequences())


@pytest.fixture(scope="module")
def video(device):
    g = golden("obb.npz")
    yolo, m = _yolo(g, TAG)
    frame = g[f"{TAG}__frame"]
    frames = [np.ascontiguousarray(np.roll(frame, (f * SHIFT[0], f * SHIFT[1]), axis=(0, 1))) for f in range(FRAMES)]
    args = dict(dtype="fp32", device=0, iou=m["iou"], imgsz=m["imgsz"])
    det = [r.obb.data.cpu().numpy() for r in yolo.predict(frames, conf=0.1, **args)]
    return yolo, frames, det, args


def _host_rows(det, streams=1):
    from drone_yolo_amd.trackers import ByteTracker

    tr = ByteTracker(rotated=True, streams=streams)
    out = [tr.update(r, stream=k % streams) if len(r) else np.zeros((0, 9), dtype=np.float32) for k, r in enumerate(det)]
    assert tr.min_margin >= M  # otherwise the device and the host path may legitimately part: pick another shift
    return out


def _data(results):
    return [r.obb.data.cpu().numpy() for r in results]


def test_track_returns_tracked_obb_results_equal_to_the_host_tracker(video):
    yolo, frames, det, args = video
    for f, r in enumerate(det):
        assert r.shape[1] == 7 and int((r[:, 5] >= 0.25).sum()) >= 5, f"frame {f}: the fixture frame gives too few detections"
    exp = _host_rows(det)
    res = yolo.track(frames, **args)
    assert len(res) == FRAMES and type(yolo.predictor).__name__ == "OBBPredictor" and yolo.predictor.tracker.rotated
    ids = []
    for f, r in enumerate(res):
        assert r.boxes is None and r.obb.is_track and r.obb.data.shape[1] == 8 and r.obb.data.is_cuda
        got = r.obb.data.cpu().numpy()
        assert np.array_equal(got[:, 5], np.round(got[:, 5])) and got[:, 5].min() >= 1 and np.array_equal(r.obb.id.cpu().numpy(), got[:, 5])
        assert_rows_match(np.concatenate([got, exp[f][:, 8:]], axis=1), exp[f], f"frame {f}")
        idx = exp[f][:, 8].astype(int)
        assert same_bits(got[:, 4], det[f][idx, 4]) and np.array_equal(got[:, 6:8], det[f][idx, 5:7])  # angle, conf and cls are the detection's at idx
        assert tuple(r.obb.xyxyxyxy.shape) == (len(got), 4, 2) and tuple(r.obb.xywhr.shape) == (len(got), 5)
        ids.append(set(got[:, 5].astype(int).tolist()))
    assert len(set.intersection(*ids)) >= 5  # ids stay with their objects over the whole video
    host = yolo.track(frames, device_track=False, **args)
    assert not hasattr(yolo.predictor.tracker, "bufs")
    for f in range(FRAMES):
        assert host[f].obb.is_track
        assert_rows_match(np.concatenate([host[f].obb.data.cpu().numpy(), exp[f][:, 8:]], axis=1), exp[f], f"host frame {f}")


def test_persist_continues_ids_and_a_new_call_restarts_them(video):
    yolo, frames, det, args = video
    whole = _data(yolo.track(frames, **args))
    first = yolo.track(frames[:4], **args)
    # frames without detections never reach the tracker (trackers/track.py:79-80): they keep their plain, empty 7-column result, and
    # the tracks go on behind them as if they had not been there
    empty = yolo.track(frames[:2], persist=True, conf=0.9999, **args)
    for r in empty:
        assert r.boxes is None and not r.obb.is_track and r.obb.id is None and tuple(r.obb.data.shape) == (0, 7)
    second = yolo.track(frames[4:], persist=True, **args)
    for a, b in zip(whole, list(first) + list(second)):
        assert same_bits(a, b.obb.data.cpu().numpy())
    streamed = yolo.track(frames, batch=3, **args)  # a source longer than one batch: the tracker goes on from batch to batch (3 + 3 + 2 frames)
    assert len(streamed) == FRAMES
    for a, b in zip(whole, streamed):
        assert same_bits(a, b.obb.data.cpu().numpy())
    gen = yolo.track(frames, stream=True, batch=2, **args)
    assert not isinstance(gen, list)
    for a, b in zip(whole, list(gen)):
        assert same_bits(a, b.obb.data.cpu().numpy())
    restarted = yolo.track(frames[4:], **args)  # persist=False: frame 1 of a new video, every high detection a track at once, ids from 1
    got = restarted[0].obb.data.cpu().numpy()
    assert got[:, 5].min() == 1 and int((det[4][:, 5] >= 0.25).sum()) == len(got) == int(got[:, 5].max())


def test_two_streams_equal_two_single_stream_runs(video):
    yolo, frames, det, args = video
    with pytest.raises(ValueError, match="track_streams"):
        yolo.track(frames[:7], track_streams=2, **args)
    a, b = frames[:4], frames[4:]  # two cameras: image k of the batch is stream k % 2
    mixed = [f for pair in zip(a, b) for f in pair]
    two = _data(yolo.track(mixed, track_streams=2, **args))
    one_a, one_b = _data(yolo.track(a, **args)), _data(yolo.track(b, **args))
    for f in range(4):
        assert same_bits(two[2 * f], one_a[f]) and same_bits(two[2 * f + 1], one_b[f]), f"time step {f}"


def test_predict_after_track_returns_plain_rows(video):
    yolo, frames, det, args = video
    yolo.track(frames, **args)
    res = yolo.predict(frames, conf=0.1, **args)
    for r, d in zip(res, det):
        assert not r.obb.is_track and r.obb.id is None and r.obb.data.shape[1] == 7 and same_bits(r.obb.data.cpu().numpy(), d)


def test_refusals_and_settings(video):
    yolo, frames, det, args = video
    with pytest.raises(FileNotFoundError, match="botsort.yaml"):  # as for a detection model: only cfg/trackers/bytetrack.yaml exists
        yolo.track(frames[:1], tracker="botsort.yaml", **args)
    with pytest.raises(NotImplementedError, match="^track with tile"):
        yolo.track(frames[:1], tile=64, **args)
    with pytest.raises(NotImplementedError, match="^track with a float BCHW tensor"):
        yolo.track(torch.zeros(1, 3, 64, 96), **args)
    small = yolo.track(frames[:2], max_tracks=4, **args)  # capacity: four slots, the rest is counted
    assert len(small[0]) == 4 and small[0].obb.is_track and int(yolo.predictor.tracker.overflow[0]) >= int((det[0][:, 5] >= 0.25).sum()) - 4 > 0
