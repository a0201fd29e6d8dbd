"""GPU: YOLO.track end to end — a model built from tests/golden/e2e.npz as the API tests build theirs, a short "video" made by shifting
one fixture image a few pixels per frame, the tracker behind the NMS on the device and on the host, persist / reset, predict afterwards."""
import numpy as np
import pytest
import torch

import drone_yolo_amd as D
from tests._track_util import assert_rows_match
from tests._util import golden
from tests.test_model_gpu import _build

pytestmark = pytest.mark.gpu
TAG, IMAGE, SHIFT, FRAMES = "n128", 0, (4, 4), 8  # fixture, its image, (rows, columns) shifted per frame
ARGS = dict(dtype="fp32", device=0)


@pytest.fixture(scope="module")
def video(device):
    m, d, sd, model, x = _build(TAG, golden("e2e.npz"), device)
    yolo = D.YOLO(m["yaml"])
    yolo.model = model
    frames = torch.stack([torch.roll(x[IMAGE], shifts=(f * SHIFT[0], f * SHIFT[1]), dims=(1, 2)) for f in range(FRAMES)])
    det = [r.boxes.data.cpu().numpy() for r in yolo.predict(frames, conf=0.1, **ARGS)]
    return yolo, frames, det


def _host_rows(det):
    from drone_yolo_amd.trackers import ByteTracker

    tr = ByteTracker()
    out = [tr.update(r) if len(r) else np.zeros((0, 8), dtype=np.float32) for r in det]
    assert tr.min_margin >= 1e-5  # otherwise the device and the host path may legitimately part: pick another image
    return out


def test_track_returns_tracked_results_equal_to_the_host_tracker(video):
    yolo, frames, det = video
    for f, r in enumerate(det):
        assert int((r[:, 4] >= 0.25).sum()) >= 5, f"frame {f}: the fixture image gives too few detections"
    exp = _host_rows(det)
    res = yolo.track(frames, **ARGS)
    assert len(res) == FRAMES
    ids = []
    for f, r in enumerate(res):
        assert r.boxes.is_track and r.boxes.data.shape[1] == 7
        got = r.boxes.data.cpu().numpy()
        assert np.array_equal(got[:, 4], np.round(got[:, 4])) and got[:, 4].min() >= 1
        assert_rows_match(np.concatenate([got, exp[f][:, 7:]], axis=1), exp[f], f"frame {f}")
        assert np.array_equal(got[:, 5:7], det[f][exp[f][:, 7].astype(int), 4:6])  # conf and cls are the detection's at idx
        ids.append(set(got[:, 4].astype(int).tolist()))
        assert r.summary()[0]["track_id"] == int(got[0, 4])
    assert len(set.intersection(*ids)) >= 5  # ids stay with their objects over the whole video
    host = yolo.track(frames, device_track=False, **ARGS)
    for f in range(FRAMES):
        assert host[f].boxes.is_track
        assert_rows_match(np.concatenate([host[f].boxes.data.cpu().numpy(), exp[f][:, 7:]], axis=1), exp[f], f"host frame {f}")


def test_persist_continues_ids_and_a_new_call_restarts_them(video):
    yolo, frames, det = video
    whole = [r.boxes.data.cpu().numpy() for r in yolo.track(frames, **ARGS)]
    first = yolo.track(frames[:4], **ARGS)
    second = yolo.track(frames[4:], persist=True, **ARGS)
    for a, b in zip(whole, list(first) + list(second)):
        assert np.array_equal(a, b.boxes.data.cpu().numpy())
    streamed = yolo.track(frames, batch=3, **ARGS)  # a source longer than one batch: the tracker goes on from batch to batch (3 + 3 + 2 frames)
    assert len(streamed) == FRAMES
    for a, b in zip(whole, streamed):
        assert np.array_equal(a, b.boxes.data.cpu().numpy())
    restarted = yolo.track(frames[4:], **ARGS)  # persist=False: frame 1 of a new video, every detection a track at once, ids from 1
    got = restarted[0].boxes.data.cpu().numpy()
    assert got[:, 4].min() == 1 and int((det[4][:, 4] >= 0.25).sum()) == len(got) == int(got[:, 4].max())


def test_predict_after_track_returns_plain_rows(video):
    yolo, frames, det = video
    yolo.track(frames, **ARGS)
    res = yolo.predict(frames, conf=0.1, **ARGS)
    for r, d in zip(res, det):
        assert not r.boxes.is_track and r.boxes.id is None and np.array_equal(r.boxes.data.cpu().numpy(), d)


def test_streams_must_divide_the_batch(video):
    yolo, frames, det = video
    with pytest.raises(ValueError, match="track_streams"):
        yolo.track(frames[:7], track_streams=2, **ARGS)
    two = yolo.track(torch.cat([frames[:2], frames[:2]]).contiguous()[[0, 2, 1, 3]], track_streams=2, **ARGS)  # two cameras showing the same video
    assert np.array_equal(two[0].boxes.data.cpu().numpy(), two[1].boxes.data.cpu().numpy())
    assert np.array_equal(two[2].boxes.data.cpu().numpy(), two[3].boxes.data.cpu().numpy())
