"""CPU: the host ByteTrack with ``rotated=True`` (drone_yolo_amd.trackers.ByteTracker) against the rows the reference's BYTETracker returned
for oriented detections on the sequences of tests/golden/track_obb.npz (tools/make_track_obb_golden.py), the fixture's own witness that
hulls are not enough, the class's reset / stream semantics, the row widths, the argument checks of the four dy_track_*_rotated entry points
(the LDS bound among them), the refusals ``YOLO.track`` keeps for ``-obb`` models, and the margins of the seeds the GPU test runs."""
import ctypes

import numpy as np
import pytest
import torch

from tests._track_obb_util import GPU_SEEDS, assert_rows_match, hull_rows, margin_all, random_sequence, sequences

SEQ = sequences()
M = margin_all(SEQ)


def _frame(s, f):
    return s["rows"][f, : s["counts"][f]]


@pytest.mark.parametrize("name", sorted(SEQ))
def test_host_rotated_tracker_matches_reference(name):
    from drone_yolo_amd.trackers import ByteTracker

    s = SEQ[name]
    tr = ByteTracker(s["cfg"], frame_rate=s["frame_rate"], rotated=True)
    for f in range(len(s["counts"])):
        got = tr.update(_frame(s, f))
        assert_rows_match(got, s["out"][f, : s["out_counts"][f]], f"{name} frame {f}")
    assert s["margin"] >= 1e-5 and tr.min_margin >= s["margin"]  # what the recording tool asserted of the reference's costs holds for this path's
    assert int(tr.overflow[0]) == 0


def test_turning_is_not_reproduced_by_an_iou_tracker_on_hulls():
    """The fixture's witness: boxes crossed over one centre have one hull; a tracker comparing hulls hands out other ids."""
    from drone_yolo_amd.trackers import ByteTracker

    s = SEQ["turning"]
    assert all((np.maximum(r[:, 2], r[:, 3]) >= 4 * np.minimum(r[:, 2], r[:, 3])).all() for r in (_frame(s, f) for f in range(len(s["counts"]))))
    angles = np.concatenate([_frame(s, f)[:, 4] for f in range(len(s["counts"]))])
    assert (angles < 0.1).any() and (angles > np.pi / 2 - 0.1).any() and (angles >= 0).all() and (angles < np.pi / 2).all()  # through the wrap
    tr = ByteTracker(s["cfg"], frame_rate=s["frame_rate"])
    differs = 0
    for f in range(len(s["counts"])):
        got = tr.update(hull_rows(_frame(s, f)))
        exp = s["out"][f, : s["out_counts"][f]]
        differs += {int(i): int(t) for i, t in zip(got[:, 7], got[:, 4])} != {int(i): int(t) for i, t in zip(exp[:, 8], exp[:, 5])}
    assert differs > 0


def test_reset_restarts_ids_and_continuing_keeps_them():
    from drone_yolo_amd.trackers import ByteTracker

    s = SEQ["sparse"]
    tr = ByteTracker(s["cfg"], rotated=True)
    first = [tr.update(_frame(s, f)) for f in range(6)]
    assert first[0][:, 5].min() == 1 and first[0].shape[1] == 9
    assert_rows_match(tr.update(_frame(s, 6)), s["out"][6, : s["out_counts"][6]], "continued")
    tr.reset()
    assert int(tr.frame_count[0]) == 0
    for a, f in zip(first, range(6)):
        assert np.array_equal(a, tr.update(_frame(s, f)))


def test_streams_are_independent_and_batches_interleave():
    from drone_yolo_amd.trackers import ByteTracker

    names = ["sparse", "turning", "gaps"]
    frames = min(len(SEQ[n]["counts"]) for n in names)
    width = max(SEQ[n]["rows"].shape[1] for n in names)
    rows = np.zeros((frames * 3, width, 7), dtype=np.float32)
    counts = np.zeros(frames * 3, dtype=np.int32)
    for k, n in enumerate(names):
        rows[k::3, : SEQ[n]["rows"].shape[1]] = SEQ[n]["rows"][:frames]
        counts[k::3] = SEQ[n]["counts"][:frames]
    cfg = SEQ["sparse"]["cfg"]
    out, cnt = ByteTracker(cfg, streams=3, rotated=True).update_batch(rows, counts)
    assert out.shape == (frames * 3, 512, 9)
    for k, n in enumerate(names):
        single = ByteTracker(cfg, rotated=True)
        for f in range(frames):
            exp = single.update(_frame(SEQ[n], f))
            assert np.array_equal(out[f * 3 + k, : cnt[f * 3 + k]], exp)
            assert not out[f * 3 + k, cnt[f * 3 + k] :].any()
    with pytest.raises(ValueError):
        ByteTracker(cfg, streams=2, rotated=True).update_batch(rows[:3], counts[:3])


def test_row_widths_are_checked():
    from drone_yolo_amd.trackers import ByteTracker

    six, seven = np.zeros((3, 6), np.float32), np.zeros((3, 7), np.float32)
    with pytest.raises(ValueError, match="rotated tracker takes .*7 columns"):
        ByteTracker(rotated=True).update(six)
    with pytest.raises(ValueError, match="plain tracker takes .*6 columns"):
        ByteTracker().update(seven)
    with pytest.raises(ValueError, match="7 columns"):
        ByteTracker(rotated=True).update_batch(six[None], np.array([3]))
    with pytest.raises(ValueError, match="6 columns"):
        ByteTracker().update_batch(seven[None], np.array([3]))
    assert ByteTracker(rotated=True).update(np.zeros((0, 7), np.float32)).shape == (0, 9)
    assert ByteTracker().update(np.zeros((0, 6), np.float32)).shape == (0, 8)


def test_nan_angle_and_zero_width_leave_the_other_tracks_alone():
    from drone_yolo_amd.trackers import ByteTracker

    s = SEQ["sparse"]
    plain, odd = ByteTracker(s["cfg"], rotated=True), ByteTracker(s["cfg"], rotated=True)
    for f in range(8):
        rows = _frame(s, f)
        extra = np.array([[900.0 + f, 40.0, 50.0, 20.0, np.nan, 0.9, 1.0], [40.0, 650.0 - f, 0.0, 30.0, 0.3, 0.85, 2.0]], np.float32)
        a, b = plain.update(rows), odd.update(np.concatenate([rows, extra]))
        keep = b[:, 8] < len(rows)
        assert np.array_equal(a[:, :5], b[keep][:, :5]) and np.array_equal(a[:, 6:], b[keep][:, 6:]), f"frame {f}"  # (ids shift: the two start tracks too)
        assert np.isnan(b[~keep][:, 4]).sum() == (1 if f == 0 else 0)  # the NaN box is a track of frame 1 only: it matches nothing afterwards


def test_rotated_entry_points_validate_without_gpu():
    import drone_yolo_amd._lib as L

    h = L.lib()
    assert h.dy_track_state_bytes_rotated(0, 512) == -1 and h.dy_track_state_bytes_rotated(1, 0) == -1 and h.dy_track_state_bytes_rotated(1, 511) == -1
    assert h.dy_track_workspace_bytes_rotated(0, 512, 300) == -1 and h.dy_track_workspace_bytes_rotated(1, 512, 0) == -1
    assert h.dy_track_workspace_bytes_rotated(1, 512, 1025) == -1 and b"max_det" in h.dy_last_error_string()
    one, many = h.dy_track_state_bytes_rotated(1, 512), h.dy_track_state_bytes_rotated(3, 512)
    assert one == h.dy_track_state_bytes(1, 512) + 512 * 4 and many == 3 * one  # the angle: one more fp32 per slot
    assert h.dy_track_workspace_bytes_rotated(2, 512, 300) == 2 * h.dy_track_workspace_bytes_rotated(1, 512, 300) > 0
    assert h.dy_track_reset_rotated(None, 1, 512, None) == -1 and b"null" in h.dy_last_error_string()
    d = L.TrackDesc()
    assert h.dy_track_step_rotated(ctypes.byref(d), None) == -1 and b"null" in h.dy_last_error_string()
    assert h.dy_track_step_rotated(None, None) == -1
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    d.rows = d.counts = d.state = d.workspace = d.out = d.out_count = p
    assert h.dy_track_step_rotated(ctypes.byref(d), None) == -1 and b"frames" in h.dy_last_error_string()  # zero sizes
    d.frames, d.streams, d.max_det, d.max_tracks = 1, 1, 300, 512
    assert h.dy_track_step_rotated(ctypes.byref(d), None) == -4  # DY_ERR_WORKSPACE: state_bytes / workspace_bytes are still 0
    assert b"dy_track_state_bytes_rotated" in h.dy_last_error_string()
    d.state_bytes = h.dy_track_state_bytes(1, 512)  # the axis-aligned state is too small
    assert h.dy_track_step_rotated(ctypes.byref(d), None) == -4
    d.state_bytes = one
    assert h.dy_track_step_rotated(ctypes.byref(d), None) == -4 and b"workspace" in h.dy_last_error_string()
    d.max_tracks = 511
    assert h.dy_track_step_rotated(ctypes.byref(d), None) == -1 and b"even" in h.dy_last_error_string()
    d.max_tracks, d.max_time_lost = 512, -1
    assert h.dy_track_step_rotated(ctypes.byref(d), None) == -1 and b"max_time_lost" in h.dy_last_error_string()


def test_rotated_lds_bound():
    """100 bytes of LDS per slot, 72 per detection, 64 more; 160 KB at most."""
    import drone_yolo_amd._lib as L

    h = L.lib()
    buf = (ctypes.c_double * 64)()
    d = L.TrackDesc()
    d.rows = d.counts = d.state = d.workspace = d.out = d.out_count = ctypes.cast(buf, ctypes.c_void_p)
    d.frames, d.streams = 1, 1
    for tracks, inside in ((1024, 852), (512, 1024), (2, 1024), (1022, 855)):
        assert tracks * 100 + inside * 72 + 64 <= 160 * 1024
        d.max_tracks, d.max_det = tracks, inside
        assert h.dy_track_step_rotated(ctypes.byref(d), None) == -4, (tracks, inside)  # past the LDS check, up to the workspace error
    for tracks, outside in ((1024, 853), (1024, 1024), (1022, 856)):
        assert tracks * 100 + outside * 72 + 64 > 160 * 1024
        d.max_tracks, d.max_det = tracks, outside
        assert h.dy_track_step_rotated(ctypes.byref(d), None) == -1
        msg = h.dy_last_error_string()
        assert b"LDS" in msg and str(tracks).encode() in msg and str(outside).encode() in msg, msg
    d.max_tracks, d.max_det = 1024, 1023  # 92 and 68 bytes: the axis-aligned bound is what it was
    assert h.dy_track_step(ctypes.byref(d), None) == -4
    d.max_det = 1024
    assert h.dy_track_step(ctypes.byref(d), None) == -1 and b"LDS" in h.dy_last_error_string()
    assert 512 * 100 + 300 * 72 + 64 == 72864  # the defaults, as include/dyolo.h states them


def test_track_desc_layout_is_unchanged(tmp_path):
    import os
    import subprocess

    import drone_yolo_amd._lib as L
    from tests._util import ROOT

    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dyolo.h"\nint main(){printf("%zu %zu %zu %zu\\n", sizeof(dy_track_desc), '
                   'offsetof(dy_track_desc, out), offsetof(dy_track_desc, frames), offsetof(dy_track_desc, max_time_lost));return 0;}\n')
    exe = tmp_path / "s"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(L.TrackDesc), L.TrackDesc.out.offset, L.TrackDesc.frames.offset, L.TrackDesc.max_time_lost.offset] == [104, 48, 64, 100]


def test_track_refusals_for_obb_models():
    from drone_yolo_amd import YOLO

    y = YOLO("yolov8n-obb.yaml")
    frame = np.zeros((64, 64, 3), np.uint8)
    with pytest.raises(NotImplementedError, match=r"^track with a float BCHW tensor.*uint8 HWC"):
        y.track(torch.zeros(1, 3, 64, 64))
    with pytest.raises(NotImplementedError, match=r"^track with tile"):
        y.track([frame], tile=64)
    with pytest.raises(NotImplementedError, match=r"^track with tile"):
        y.track(torch.zeros(1, 3, 64, 64), tile=64)
    with pytest.raises(NotImplementedError, match="augment"):
        y.track([frame], augment=True)
    assert y.predictor is None and all(p.device.type == "cpu" for p in y.model.parameters())


def test_botsort_is_refused_for_rotated_trackers_too():
    from drone_yolo_amd.trackers import ByteTracker, load_tracker_cfg

    c = load_tracker_cfg("bytetrack.yaml")
    with pytest.raises(NotImplementedError, match="cv2"):
        ByteTracker(dict(vars(c), tracker_type="botsort"), rotated=True)
    for rotated in (False, True):  # a settings file that does not exist: the same error for both (tests/test_track_obb_api_gpu.py: through YOLO.track)
        with pytest.raises(FileNotFoundError, match="botsort.yaml"):
            ByteTracker("botsort.yaml", rotated=rotated)


def test_every_gpu_seed_keeps_the_margin_on_the_host():
    """The random sequences of tests/test_track_obb_gpu.py, all of them: no cost within M of the threshold it is compared with, so the
    device's own cosf / sinf / logf / expf cannot change a verdict."""
    from drone_yolo_amd.trackers import ByteTracker

    assert M >= 1e-5 and len(GPU_SEEDS) >= 6
    sizes = []
    for seed in GPU_SEEDS:
        tr = ByteTracker(max_det=300, rotated=True)
        frames = random_sequence(seed)
        for rows in frames:
            assert rows.shape[1] == 7 and len(rows) <= 300 and (rows[:, 4] >= -np.pi / 4).all() and (rows[:, 4] < 3 * np.pi / 4).all()
            tr.update(rows)
        assert tr.min_margin >= M, f"seed {seed}: a cost lies {tr.min_margin} from its threshold, M is {M}"
        sizes.append(max(map(len, frames)))
    assert max(sizes) > 200 and any(min(map(len, random_sequence(s))) == 0 for s in GPU_SEEDS)
