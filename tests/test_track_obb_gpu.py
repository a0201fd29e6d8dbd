"""GPU: the dy_track_step_rotated kernel (drone_yolo_amd.trackers.DeviceByteTracker with ``rotated=True``) against the reference's rows of
tests/golden/track_obb.npz, its F > 1 and S > 1 forms against its own one-image-per-launch run (bit-identical), seeded random rotated
sequences against the host path (every seed keeps the margin: tests/test_track_obb_host.py), and the shapes where the kernel changes its
path: lane and thread strides, one detection, an empty frame, capacity, the largest pair the LDS bound admits, a NaN angle, a zero width."""
import numpy as np
import pytest
import torch

from tests._track_obb_util import GPU_SEEDS, assert_rows_match, margin_all, random_sequence, same_bits, sequences

pytestmark = pytest.mark.gpu
SEQ = sequences()
M = margin_all(SEQ)
_single = {}  # name -> the one-image-per-launch rows of the device tracker, computed once and shared


def _padded(frames, max_det):
    rows = np.zeros((len(frames), max_det, 7), dtype=np.float32)
    counts = np.zeros(len(frames), dtype=np.int32)
    for f, r in enumerate(frames):
        rows[f, : len(r)], counts[f] = r, len(r)
    return rows, counts


def _frames_of(name):
    s = SEQ[name]
    return [s["rows"][f, : s["counts"][f]] for f in range(len(s["counts"]))]


def _run(device, cfg, frames, per_launch, max_det=300, streams=1, max_tracks=512, first=0):
    """The frames (image k = stream k % streams) through a fresh rotated device tracker, `per_launch` time steps per launch (`first` in the
    first launch when given) -> list of (k, 9) arrays.  Checked on the way: rows at and beyond the count are zero, and every row carries
    the angle of the detection at its idx bit for bit (a row out is a track matched or started in this frame)."""
    from drone_yolo_amd.trackers import DeviceByteTracker

    tr = DeviceByteTracker(cfg, streams=streams, max_det=max_det, max_tracks=max_tracks, device=device, rotated=True)
    rows, counts = _padded(frames, max_det)
    rows_d, counts_d = torch.from_numpy(rows).to(device), torch.from_numpy(counts).to(device)
    out = []
    step = per_launch * streams
    cuts = list(range(first * streams, len(frames), step)) + [len(frames)]
    for lo, hi in zip(([0] if first else []) + cuts[:-1], cuts if first else cuts[1:]):
        o, c = tr.update_batch(rows_d[lo:hi], counts_d[lo:hi])
        o, c = o.cpu().numpy(), c.cpu().numpy()
        assert o.shape == (hi - lo, max_tracks, 9)
        assert (o.reshape(len(c), -1).view(np.uint32)[np.arange(o.shape[1] * 9)[None, :] >= c[:, None] * 9] == 0).all()
        for i in range(len(c)):
            r = o[i, : c[i]].copy()
            assert same_bits(r[:, 4], rows[lo + i, r[:, 8].astype(int), 4]), f"image {lo + i}: a row's angle is not its detection's"
            out.append(r)
    return out, tr


def _single_run(device, name):
    if name not in _single:
        _single[name] = _run(device, SEQ[name]["cfg"], _frames_of(name), 1)[0]
    return _single[name]


def _host(cfg, frames, max_tracks=512):
    """The host rotated tracker on the frames; asserts that no cost came within M of a threshold (the two paths may part there)."""
    from drone_yolo_amd.trackers import ByteTracker

    host = ByteTracker(cfg, max_det=1024, max_tracks=max_tracks, rotated=True)
    exp = [host.update(r) for r in frames]
    assert host.min_margin >= M, f"a cost lies {host.min_margin} from its threshold, M is {M}: pick other inputs"
    return exp, host


@pytest.mark.parametrize("name", sorted(SEQ))
def test_device_rotated_tracker_matches_reference(device, name):
    s = SEQ[name]
    got = _single_run(device, name)
    for f in range(len(s["counts"])):
        assert_rows_match(got[f], s["out"][f, : s["out_counts"][f]], f"{name} frame {f}")


@pytest.mark.parametrize("name", sorted(SEQ))
def test_eight_frames_per_launch_is_bit_identical(device, name):
    frames = _frames_of(name)
    many, tr = _run(device, SEQ[name]["cfg"], frames, 8, first=0 if len(frames) % 8 else 3)  # launches of 8 and a remainder
    assert len(many) == len(frames)
    for a, b in zip(many, _single_run(device, name)):
        assert same_bits(a, b)
    assert int(tr.frame_count[0]) == int((SEQ[name]["counts"] > 0).sum()) and int(tr.overflow[0]) == 0


def test_three_interleaved_streams_are_bit_identical(device):
    names = ["sparse", "turning", "gaps"]
    n = min(len(SEQ[k]["counts"]) for k in names)
    frames = [_frames_of(k)[f] for f in range(n) for k in names]
    cfg = SEQ["sparse"]["cfg"]
    out, _ = _run(device, cfg, frames, 5, streams=3)
    for k, name in enumerate(names):
        single = _single_run(device, name) if SEQ[name]["cfg"] == cfg else _run(device, cfg, _frames_of(name)[:n], 1)[0]
        for f in range(n):
            assert same_bits(out[f * 3 + k], single[f]), f"{name} frame {f}"


@pytest.mark.parametrize("seed", GPU_SEEDS)
def test_random_rotated_sequences_match_the_host_path(device, seed):
    frames = random_sequence(seed)
    exp, host = _host("bytetrack.yaml", frames)
    got, tr = _run(device, "bytetrack.yaml", frames, 10)
    for f in range(len(frames)):
        assert_rows_match(got[f], exp[f], f"seed {seed} frame {f}")
    assert int(tr.overflow[0]) == int(host.overflow[0])


def _grid(n, frames, seed, pitch=64.0, drop=7):
    """n objects on a square grid `pitch` apart (40 x 10 boxes at random angles: neighbours do not overlap, so every cost is far from its
    threshold), drifting a pixel and turning 0.02 rad per frame; frame f leaves out every `drop`-th object, offset by f."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(n)))
    xy = np.stack(np.meshgrid(np.arange(side), np.arange(side)), axis=-1).reshape(-1, 2)[:n] * pitch + 40
    th = rng.uniform(-np.pi / 4, 3 * np.pi / 4, n)
    conf = np.linspace(0.95, 0.3, n)
    out = []
    for f in range(frames):
        keep = (np.arange(n) + f) % drop != 0 if drop else np.ones(n, bool)
        t = (th + 0.02 * f + np.pi / 4) % np.pi - np.pi / 4
        rows = np.stack([xy[:, 0] + f, xy[:, 1] + 0.5 * f, np.full(n, 40.0), np.full(n, 10.0), t, conf, np.arange(n) % 3], axis=1)[keep]
        out.append(rows.astype(np.float32))
    return out


@pytest.mark.parametrize("n,max_det,max_tracks", [(100, 128, 512), (324, 300, 512), (5, 852, 1024)],
                         ids=["lane-stride", "thread-stride", "largest-lds-pair"])
def test_shapes_against_the_host_path(device, n, max_det, max_tracks):
    """More than 64 / more than 256 tracks and detections; the largest (max_tracks, max_det) the LDS bound admits with a handful of
    objects; in each: a frame without detections between full ones, and a frame with exactly one detection."""
    frames = _grid(n, 4, seed=n)
    frames = frames[:2] + [np.zeros((0, 7), np.float32)] + frames[2:] + [frames[3][:1]]
    exp, host = _host("bytetrack.yaml", frames, max_tracks=max_tracks)
    got, tr = _run(device, "bytetrack.yaml", frames, 3, max_det=max_det, max_tracks=max_tracks)
    assert max(map(len, frames)) <= max_det and min(len(exp[0]), len(frames[0])) > {100: 64, 324: 256, 5: 3}[n] and len(exp[2]) == 0 and len(exp[-1]) == 1
    for f in range(len(frames)):
        assert_rows_match(got[f], exp[f], f"frame {f}")
    assert int(tr.overflow[0]) == 0 and int(tr.frame_count[0]) == 5


def test_capacity(device):
    frames = _grid(100, 3, seed=3, drop=0)
    exp, host = _host("bytetrack.yaml", frames, max_tracks=32)
    out, tr = _run(device, "bytetrack.yaml", frames, 1, max_tracks=32)
    assert int(tr.overflow[0]) == int(host.overflow[0]) > 0
    for f, o in enumerate(out):
        assert len(o) == 32 and np.array_equal(o[:, 5], np.arange(1, 33)) and np.array_equal(o[:, 8], np.arange(32))
        assert_rows_match(o, exp[f], f"frame {f}")


def test_nan_angle_and_zero_width_against_the_host_path(device):
    s = SEQ["sparse"]
    frames, plain = [], _frames_of("sparse")[:8]
    for f, rows in enumerate(plain):
        extra = np.array([[900.0 + f, 40.0, 50.0, 20.0, np.nan, 0.9, 1.0], [40.0, 650.0 - f, 0.0, 30.0, 0.3, 0.85, 2.0]], np.float32)
        frames.append(np.concatenate([rows, extra]))
    exp, _ = _host(s["cfg"], frames)
    got, _ = _run(device, s["cfg"], frames, 4)
    for f in range(len(frames)):
        assert_rows_match(got[f], exp[f], f"frame {f}")
        ordinary = got[f][got[f][:, 8] < len(plain[f])]  # the ordinary tracks are those of the sequence without the two boxes
        ref = _single_run(device, "sparse")[f]
        assert same_bits(ordinary[:, :5], ref[:, :5]) and same_bits(ordinary[:, 6:], ref[:, 6:]), f"frame {f}"
    assert np.isnan(got[0][:, 4]).sum() == 1 and not any(np.isnan(g[:, 4]).any() for g in got[1:])


def test_row_widths_and_the_lds_bound_are_refused_before_a_launch(device):
    from drone_yolo_amd.trackers import DeviceByteTracker

    tr = DeviceByteTracker(max_det=16, device=device, rotated=True)
    with pytest.raises(ValueError, match="7"):
        tr.update_batch(torch.zeros((1, 16, 6), device=device), torch.zeros(1, dtype=torch.int32, device=device))
    with pytest.raises(ValueError, match="6"):
        DeviceByteTracker(max_det=16, device=device).update_batch(torch.zeros((1, 16, 7), device=device), torch.zeros(1, dtype=torch.int32, device=device))
    big = DeviceByteTracker(max_det=853, max_tracks=1024, device=device, rotated=True)
    with pytest.raises(Exception, match="max_tracks 1024 with max_det 853"):
        big.update_batch(torch.zeros((1, 853, 7), device=device), torch.zeros(1, dtype=torch.int32, device=device))
