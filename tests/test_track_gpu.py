"""GPU: the dy_track_step kernel (drone_yolo_amd.trackers.DeviceByteTracker) against the reference's rows of tests/golden/track.npz, its
F > 1 and S > 1 forms against its own one-image-per-launch run (bit-identical), seeded random sequences against the host path, and the
behaviour at capacity."""
import numpy as np
import pytest
import torch

from tests._track_util import assert_rows_match, random_sequence, sequences

pytestmark = pytest.mark.gpu
SEQ = sequences()
_single = {}  # name -> the one-image-per-launch rows of the device tracker, computed once and shared


def _padded(frames, max_det):
    rows = np.zeros((len(frames), max_det, 6), dtype=np.float32)
    counts = np.zeros(len(frames), dtype=np.int32)
    for f, r in enumerate(frames):
        rows[f, : len(r)], counts[f] = r, len(r)
    return rows, counts


def _frames_of(name):
    s = SEQ[name]
    return [s["rows"][f, : s["counts"][f]] for f in range(len(s["counts"]))]


def _run(device, cfg, frames, per_launch, max_det=300, streams=1, max_tracks=512, first=0):
    """The frames (image k = stream k % streams) through a fresh device tracker, `per_launch` time steps per launch (`first` in the first
    launch when given) -> list of (k, 8) arrays."""
    from drone_yolo_amd.trackers import DeviceByteTracker

    tr = DeviceByteTracker(cfg, streams=streams, max_det=max_det, max_tracks=max_tracks, device=device)
    rows, counts = _padded(frames, max_det)
    rows_d, counts_d = torch.from_numpy(rows).to(device), torch.from_numpy(counts).to(device)
    out = []
    step = per_launch * streams
    cuts = list(range(first * streams, len(frames), step)) + [len(frames)]
    for lo, hi in zip(([0] if first else []) + cuts[:-1], cuts if first else cuts[1:]):
        o, c = tr.update_batch(rows_d[lo:hi], counts_d[lo:hi])
        o, c = o.cpu().numpy(), c.cpu().numpy()
        assert (o.reshape(len(c), -1)[np.arange(o.shape[1] * 8)[None, :] >= c[:, None] * 8] == 0).all()  # rows at and beyond the count are zero
        out += [o[i, : c[i]].copy() for i in range(len(c))]
    return out, tr


def _single_run(device, name):
    if name not in _single:
        _single[name] = _run(device, SEQ[name]["cfg"], _frames_of(name), 1)[0]
    return _single[name]


@pytest.mark.parametrize("name", sorted(SEQ))
def test_device_tracker_matches_reference(device, name):
    s = SEQ[name]
    got = _single_run(device, name)
    for f in range(len(s["counts"])):
        assert_rows_match(got[f], s["out"][f, : s["out_counts"][f]], f"{name} frame {f}")


@pytest.mark.parametrize("name", sorted(SEQ))
def test_eight_frames_per_launch_is_bit_identical(device, name):
    frames = _frames_of(name)
    many, tr = _run(device, SEQ[name]["cfg"], frames, 8, first=0 if len(frames) % 8 else 3)  # launches of 8 and a remainder (40 frames: 3, 8 x 4, 5)
    assert len(many) == len(frames)
    for a, b in zip(many, _single_run(device, name)):
        assert np.array_equal(a, b)
    assert int(tr.frame_count[0]) == int((SEQ[name]["counts"] > 0).sum()) and int(tr.overflow[0]) == 0


def test_three_interleaved_streams_are_bit_identical(device):
    names = ["sparse", "flicker", "gaps"]
    n = min(len(SEQ[k]["counts"]) for k in names)
    frames = [_frames_of(k)[f] for f in range(n) for k in names]
    # one settings object per tracker: the streams share flicker's (track_buffer 4), so the single-stream runs to compare with use it too
    cfg = SEQ["flicker"]["cfg"]
    out, _ = _run(device, cfg, frames, 5, streams=3)
    for k, name in enumerate(names):
        single, _ = _run(device, cfg, _frames_of(name)[:n], 1)
        for f in range(n):
            assert np.array_equal(out[f * 3 + k], single[f]), f"{name} frame {f}"


def test_random_sequences_match_the_host_path(device):
    from drone_yolo_amd.trackers import ByteTracker

    left_out = 0
    for seed in range(20):
        frames = random_sequence(seed)
        host = ByteTracker(max_det=300)
        exp = [host.update(r) for r in frames]
        if host.min_margin < 1e-5:  # a cost within 1e-5 of its threshold: the two paths may legitimately part there
            left_out += 1
            continue
        got, tr = _run(device, "bytetrack.yaml", frames, 10)
        for f in range(len(frames)):
            assert_rows_match(got[f], exp[f], f"seed {seed} frame {f}")
        assert int(tr.overflow[0]) == int(host.overflow[0])
    assert left_out <= 2


def test_capacity(device):
    g = np.stack(np.meshgrid(np.arange(10), np.arange(10)), axis=-1).reshape(-1, 2) * 100.0 + 50
    rows = np.concatenate([g - 15, g + 15, np.linspace(0.95, 0.5, 100)[:, None], np.zeros((100, 1))], axis=1).astype(np.float32)
    frames = [rows, rows + np.float32([1, 0, 1, 0, 0, 0]), rows + np.float32([2, 0, 2, 0, 0, 0])]
    out, tr = _run(device, "bytetrack.yaml", frames, 1, max_tracks=32)
    assert int(tr.overflow[0]) > 0
    for o in out:
        assert len(o) == 32 and np.array_equal(o[:, 4], np.arange(1, 33)) and np.array_equal(o[:, 7], np.arange(32))
