"""CPU: the host ByteTrack (drone_yolo_amd.trackers.ByteTracker) against the rows the reference's BYTETracker returned on the sequences of
tests/golden/track.npz (tools/make_track_golden.py), the class's reset / stream semantics, the settings file, and the descriptor checks of
the four dy_track_* entry points."""
import ctypes

import numpy as np
import pytest

from tests._track_util import assert_rows_match, random_sequence, sequences

SEQ = sequences()


@pytest.mark.parametrize("name", sorted(SEQ))
def test_host_tracker_matches_reference(name):
    from drone_yolo_amd.trackers import ByteTracker

    s = SEQ[name]
    tr = ByteTracker(s["cfg"], frame_rate=s["frame_rate"])
    for f in range(len(s["counts"])):
        got = tr.update(s["rows"][f, : s["counts"][f]])
        assert_rows_match(got, s["out"][f, : s["out_counts"][f]], f"{name} frame {f}")
    assert tr.min_margin >= 1e-5  # what the recording tool asserted of the reference's costs holds for this path's costs too
    assert int(tr.overflow[0]) == 0


def test_reset_restarts_ids_and_continuing_keeps_them():
    from drone_yolo_amd.trackers import ByteTracker

    s = SEQ["sparse"]
    tr = ByteTracker(s["cfg"])
    first = [tr.update(s["rows"][f, : s["counts"][f]]) for f in range(6)]
    assert first[0][:, 4].min() == 1
    more = tr.update(s["rows"][6, : s["counts"][6]])  # without a reset the ids go on
    assert_rows_match(more, s["out"][6, : s["out_counts"][6]], "continued")
    tr.reset()
    assert int(tr.frame_count[0]) == 0
    again = [tr.update(s["rows"][f, : s["counts"][f]]) for f in range(6)]
    for a, b in zip(first, again):
        assert np.array_equal(a, b)


def test_streams_are_independent_and_batches_interleave():
    from drone_yolo_amd.trackers import ByteTracker

    names = ["sparse", "flicker", "gaps"]
    frames = min(len(SEQ[n]["counts"]) for n in names)
    width = max(SEQ[n]["rows"].shape[1] for n in names)
    rows = np.zeros((frames * 3, width, 6), dtype=np.float32)
    counts = np.zeros(frames * 3, dtype=np.int32)
    for k, n in enumerate(names):
        rows[k::3, : SEQ[n]["rows"].shape[1]] = SEQ[n]["rows"][:frames]
        counts[k::3] = SEQ[n]["counts"][:frames]
    cfg = SEQ["sparse"]["cfg"]
    out, cnt = ByteTracker(cfg, streams=3).update_batch(rows, counts)
    for k, n in enumerate(names):
        single = ByteTracker(cfg)
        for f in range(frames):
            exp = single.update(SEQ[n]["rows"][f, : SEQ[n]["counts"][f]])
            assert np.array_equal(out[f * 3 + k, : cnt[f * 3 + k]], exp)
    with pytest.raises(ValueError):
        ByteTracker(cfg, streams=2).update_batch(rows[:3], counts[:3])


def test_capacity_overflow_counts_and_keeps_tracking():
    from drone_yolo_amd.trackers import ByteTracker

    g = np.stack(np.meshgrid(np.arange(10), np.arange(10)), axis=-1).reshape(-1, 2) * 100.0 + 50
    rows = np.concatenate([g - 15, g + 15, np.linspace(0.95, 0.5, 100)[:, None], np.zeros((100, 1))], axis=1).astype(np.float32)
    tr = ByteTracker(max_tracks=32)
    out = tr.update(rows)
    assert len(out) == 32 and int(tr.overflow[0]) == 68 and np.array_equal(out[:, 4], np.arange(1, 33))
    for _ in range(2):
        nxt = tr.update(rows + np.float32([1, 0, 1, 0, 0, 0]))
        assert np.array_equal(nxt[:, 4], np.arange(1, 33)) and np.array_equal(nxt[:, 7], np.arange(32))


def test_random_sequences_have_margin_on_the_host():
    """The seeds of the device test: at most 2 of 20 may come within 1e-5 of a threshold (those are left out there)."""
    from drone_yolo_amd.trackers import ByteTracker

    tight = 0
    for seed in range(20):
        tr = ByteTracker(max_det=300)
        for rows in random_sequence(seed):
            tr.update(rows)
        tight += tr.min_margin < 1e-5
    assert tight <= 2


def test_settings_file_and_botsort():
    from drone_yolo_amd.trackers import ByteTracker, load_tracker_cfg
    from drone_yolo_amd.trackers.bytetrack import CFG_KEYS

    c = load_tracker_cfg("bytetrack.yaml")
    assert sorted(vars(c)) == sorted(CFG_KEYS) and len(CFG_KEYS) == 7
    assert (c.tracker_type, c.track_high_thresh, c.track_low_thresh, c.new_track_thresh, c.track_buffer, c.match_thresh, c.fuse_score) == \
        ("bytetrack", 0.25, 0.1, 0.25, 30, 0.8, True)
    with pytest.raises(NotImplementedError, match="cv2"):
        ByteTracker(dict(vars(c), tracker_type="botsort"))
    with pytest.raises(NotImplementedError):
        load_tracker_cfg({"tracker_type": "botsort"})


def test_track_entry_points_validate_without_gpu():
    import drone_yolo_amd._lib as L

    h = L.lib()
    assert h.dy_track_state_bytes(0, 512) == -1 and h.dy_track_state_bytes(1, 0) == -1 and h.dy_track_workspace_bytes(0, 512, 300) == -1
    one, many = h.dy_track_state_bytes(1, 512), h.dy_track_state_bytes(3, 512)
    assert one > 512 * (8 + 64) * 8 and many == 3 * one and h.dy_track_workspace_bytes(2, 512, 300) == 2 * h.dy_track_workspace_bytes(1, 512, 300) > 0
    assert h.dy_track_reset(None, 1, 512, None) == -1 and b"null" in h.dy_last_error_string()
    d = L.TrackDesc()
    assert h.dy_track_step(ctypes.byref(d), None) == -1 and b"null" in h.dy_last_error_string()
    assert h.dy_track_step(None, None) == -1
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    d.rows = d.counts = d.state = d.workspace = d.out = d.out_count = p
    assert h.dy_track_step(ctypes.byref(d), None) == -1 and b"frames" in h.dy_last_error_string()  # zero sizes
    d.frames, d.streams, d.max_det, d.max_tracks = 1, 1, 300, 512
    assert h.dy_track_step(ctypes.byref(d), None) == -4  # DY_ERR_WORKSPACE: state_bytes / workspace_bytes are still 0
    d.max_tracks = 511
    assert h.dy_track_step(ctypes.byref(d), None) == -1 and b"even" in h.dy_last_error_string()


def test_track_desc_layout_matches_header(tmp_path):
    import os
    import subprocess

    import drone_yolo_amd._lib as L
    from tests._util import ROOT

    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include "dyolo.h"\nint main(){printf("%zu\\n", sizeof(dy_track_desc));return 0;}\n')
    exe = tmp_path / "s"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert int(subprocess.check_output([str(exe)])) == ctypes.sizeof(L.TrackDesc)
