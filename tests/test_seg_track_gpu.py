"""GPU: ``YOLO.track`` of a segmentation model, with and without ``tile=`` -- the device tracker against the host tracker, every track's mask
against the plain predict's mask of the detection it matched, ``persist`` across calls -- and the detection model's tiled predict / track,
which share the tiled loop, against themselves through the task-neutral path."""
import numpy as np
import pytest
import torch

from tests._tile_util import block_frame
from tests._track_util import assert_rows_match
from tests._util import golden
from tests.test_seg_gpu import _yolo

pytestmark = pytest.mark.gpu
SHAPE = (200, 300)
BASE = dict(dtype="fp32", device=0, conf=0.25, iou=0.7)
# the segmentation fixture's scores lie in 0.195-0.256: ByteTrack's settings with its three score thresholds moved below them
TRACKER = "tracker_type: bytetrack\ntrack_high_thresh: 0.22\ntrack_low_thresh: 0.1\nnew_track_thresh: 0.2\ntrack_buffer: 30\nmatch_thresh: 0.8\nfuse_score: True\n"
TILED = dict(tile=128, tile_overlap=0.25, merge_iou=0.6, tile_mask_stride=2)


def _video(n=4):
    base = block_frame(4, SHAPE)
    return [np.ascontiguousarray(np.roll(base, (2 * f, 3 * f), (0, 1))) for f in range(n)]  # the frame drifting a few pixels per step


@pytest.fixture(scope="module")
def seg():
    return _yolo(golden("seg.npz"), "seg3n64x96")[0]


@pytest.mark.parametrize("tiled", [False, True], ids=["plain", "tile"])
def test_track_carries_the_matched_detections_masks(device, seg, tiled, tmp_path):
    frames = _video()
    (tmp_path / "bytetrack_low.yaml").write_text(TRACKER)
    kw = dict(**{**BASE, "conf": 0.2}, **(TILED if tiled else dict(imgsz=256)))  # (at imgsz 128 this fixture's boxes
    # degenerate to the whole image and two tracks of frame 1 tie between detections: the device and the host tracker then pick differently)
    plain = seg.predict(frames, batch=2, **kw)
    kw["tracker"] = str(tmp_path / "bytetrack_low.yaml")
    plain_masks = [r.masks.data.clone() if r.masks is not None else None for r in plain]
    plain_rows = [r.boxes.data.clone() for r in plain]
    dev, index = [], []
    for lo in (0, 2):  # two batches of two time steps, the second call going on with the first one's tracks
        dev += seg.track(frames[lo : lo + 2], persist=lo > 0, **kw)
        index += seg.predictor.last_track_index
    whole = seg.track(frames, batch=2, **kw)
    host = seg.track(frames, batch=2, device_track=False, **kw)
    assert len(dev) == len(whole) == len(host) == len(frames) and any(r.boxes.is_track for r in dev)
    for f, (d, w, h) in enumerate(zip(dev, whole, host)):
        assert d.boxes.is_track == h.boxes.is_track == w.boxes.is_track
        assert np.array_equal(d.boxes.data.cpu().numpy(), w.boxes.data.cpu().numpy()), f"persist, frame {f}"  # two calls with persist = one call
        if d.boxes.is_track:
            assert_rows_match(d.boxes.data.cpu().numpy(), h.boxes.data.cpu().numpy(), f"frame {f}")
        idx = index[f]
        assert idx.dtype == torch.int64 and len(idx) == len(d)
        if len(d):
            assert torch.equal(d.boxes.data[:, -2:], plain_rows[f][idx][:, 4:])  # a track's score and class are its detection's
            assert torch.equal(d.masks.data, plain_masks[f][idx]), f"frame {f}: a track's mask is not its detection's"
            assert torch.equal(h.masks.data, d.masks.data) and torch.equal(w.masks.data, d.masks.data)
        else:
            assert d.masks is None


def test_detection_tiled_predict_and_track_are_unchanged(device):
    """A detection model through the shared tiled loop gives what it gave before segmentation went through it: the rows of tiled predict and
    of tiled track on the drifting block frame, recorded at the parent commit (tests/golden/tile_det_parent.npz), bit for bit; no masks."""
    import drone_yolo_amd as D
    from tests.test_model_gpu import _build

    g = golden("tile_det_parent.npz")
    m, _, _, model, _ = _build("n128", golden("e2e.npz"), device)
    y = D.YOLO(m["yaml"])
    y.model = model
    frames = _video()
    kw = dict(**BASE, tile=128, tile_overlap=0.25, merge_iou=0.6)
    pred, trk = y.predict(frames, batch=2, **kw), y.track(frames, batch=2, **kw)
    assert any(r.boxes.is_track for r in trk)
    for f in range(len(frames)):
        assert pred[f].masks is None and trk[f].masks is None
        assert np.array_equal(pred[f].boxes.data.cpu().numpy(), g[f"predict_{f}"]), f"predict, frame {f}"
        assert np.array_equal(trk[f].boxes.data.cpu().numpy(), g[f"track_{f}"]), f"track, frame {f}"
