"""CPU: the oracle of the oriented-box tile merge and the public interface's refusals.

The numpy fp32 restatement of ``dy_tile_merge_rotated`` (tests/_tile_rot_util.py::merge_ref_rotated) keeps the slots a float64 greedy run
keeps, on every case the GPU tests use, and those cases keep the project's margin from the threshold (M = 8 x max |p32 - p64| over the pairs
the greedy run decides on): the kernel, whose sinf / cosf / logf / expf are not numpy's bit for bit, must then keep the same slots.  On the
chain case the greedy restatement keeps A and C where the reference's fast NMS keeps only A.  ``tile=`` on an ``-obb`` model refuses what the
rotated merge does not do by argument name, before a predictor exists or a parameter leaves the CPU."""
import functools

import numpy as np
import pytest
import torch

from drone_yolo_amd import YOLO
from tests import _obb_util as U
from tests import _tile_rot_util as T

MODES = [(n, k, a) for n, k in T.RUNS for a in (False, True)]


@functools.lru_cache(maxsize=None)
def _greedy(name, agnostic, keep):
    rows, counts, offs = T.case_rows(name)
    return T.greedy64(rows, counts, offs, T.THR, agnostic, keep)


@pytest.mark.parametrize("name,keep,agnostic", MODES, ids=[f"{n}-{k}-{'agnostic' if a else 'by_class'}" for n, k, a in MODES])
def test_restatement_keeps_what_float64_keeps_with_a_margin(name, keep, agnostic):
    F, K, md = T.CASES[name][:3]
    _, counts, _ = T.case_rows(name)
    out, cnt, idx = T.case_ref(name, agnostic, keep)
    kept, p64, p32 = _greedy(name, agnostic, keep)
    m, dist = T.margin(p64, p32, T.THR)
    print(f"{name} keep {keep} agnostic {agnostic}: kept {cnt.tolist()} of {[int(counts[f * K:(f + 1) * K].sum()) for f in range(F)]}, "
          f"{len(p64)} pairs, M = {m:.3e}, nearest pair {dist:.3e} from the threshold")
    assert len(p64) > 0 and dist >= m, f"a decided pair lies {dist} from the threshold, the margin is {m}"
    for f in range(F):
        assert np.array_equal(idx[f, : cnt[f]], kept[f]) and (idx[f, cnt[f] :] == -1).all() and (out[f, cnt[f] :] == 0).all()
    assert (cnt <= keep).all()


def test_cases_are_what_they_are_for():
    for name, (F, K, md, nc, hw, tile, overlap, _) in T.CASES.items():
        rows, counts, offs = T.case_rows(name)
        assert rows.shape == (F * K, md, 7) and len(offs) == K and K * md <= 32768
        per_frame = counts.reshape(F, K).sum(1)
        for f in range(F):  # distinct scores within a frame
            s = np.concatenate([rows[f * K + k, : counts[f * K + k], 5] for k in range(K)])
            assert len(np.unique(s)) == len(s)
        if K > 1:
            assert (offs[:, 0] != offs[:, 1]).any()
        if name == "ragged":
            assert per_frame[1] == 0 and (counts.reshape(F, K)[[0, 2]].min(1) == 0).all() and counts.max() == md
            out, cnt, _ = T.case_ref(name, False, 16)
            assert (cnt[[0, 2]] == 16).all()  # truncated in the middle of a chunk
        if name == "chunks":
            assert tuple(per_frame) == T.CHUNK_TOTALS
        if name == "12k":
            assert K * md == 12000 and T.case_ref(name, False, 4096)[1][0] > 1000
        if name == "limit":
            assert K * md == 32700
        cnt = T.case_ref(name, False, 1000)[1]
        assert K == 1 or ((cnt < per_frame) | (per_frame == 0)).all(), "every frame with rows loses cross-tile duplicates"


@pytest.mark.parametrize("thr", [1e-3, 0.05, T.THR, 0.7, 0.999, 1.0])
def test_pairs_the_kernel_does_not_finish_never_reach_the_threshold(thr):
    """The kernel skips the second half of the expression for a pair whose distance terms exceed ``far_bound(thr)`` (summed determinant
    positive).  Over 400,000 seeded pairs -- sizes from degenerate to 2,000 px, distances from 0 to 6,000 px -- every such pair's ProbIoU in the
    restatement lies below thr (or is NaN, which does not suppress), by at least 1e-4; and the bound does fire."""
    rng = np.random.default_rng(7)
    n = 400_000
    def boxes():
        wh = np.where(rng.random((n, 2)) < 0.05, 0.0, 10 ** rng.uniform(-2, 3.3, (n, 2)))
        return T.cov_rows32(rng.uniform(0, 4000, n) * rng.integers(0, 2, n), rng.uniform(0, 4000, n) * rng.integers(0, 2, n), wh[:, 0], wh[:, 1], rng.uniform(-1, 2.5, n))
    r1, r2 = boxes(), boxes()
    t12, det = T.distance_terms32(r1, r2)
    skipped = (det > 0) & (t12 > T.far_bound(thr))
    p = T.probiou32(r1, r2)
    assert skipped.sum() > n // 10 and (~skipped).sum() > n // 100
    assert not (p[skipped] >= np.float32(thr) - np.float32(1e-4)).any()
    assert T.far_bound(0.0) == np.inf and T.far_bound(5e-4) == np.inf


def test_float64_row_form_is_probiou64():
    rows, counts, offs = T.case_rows("one_tile")
    box = rows[0, :40, :5].astype(np.float64)
    full = U.probiou64(box)
    for i in (0, 7, 39):
        assert np.array_equal(T.probiou64_rows(box[i], box), full[i])


@pytest.mark.parametrize("name", T.HAND_CASES)
def test_hand_cases(name):
    rows, counts, offs, expect = T.hand_case(name)
    for agnostic, slots in expect.items():
        out, cnt, idx = T.merge_ref_rotated(rows, counts, offs, T.HAND_FRAME, T.THR, agnostic, 16)
        assert idx[0, : cnt[0]].tolist() == slots, (name, agnostic)
        if name != "degenerate":  # (alone in their classes: no pair is decided)
            kept, p64, p32 = T.greedy64(rows, counts, offs, T.THR, agnostic, 16)
            m, dist = T.margin(p64, p32, T.THR)
            assert kept[0].tolist() == slots and dist >= m
    if name == "chain":  # greedy keeps A and C; the reference's fast NMS (a suppressed row still suppresses) keeps only A
        p = U.probiou64(np.asarray(U.chain_boxes(U.CHAIN_D)))
        assert U.fast_nms(p, T.THR) == [0] and U.greedy_nms(p, T.THR) == [0, 2]
    if name == "offsets":  # with (ox, oy) the wrong way round the two views would be two objects
        swapped = T.merge_ref_rotated(rows, counts, offs[:, ::-1], T.HAND_FRAME, T.THR, False, 16)
        assert swapped[1][0] == 2
    if name == "clamp":
        out = T.merge_ref_rotated(rows, counts, offs, T.HAND_FRAME, T.THR, False, 16)[0][0]
        assert out[0, 0] == 320.0 and out[1, 1] == 0.0 and tuple(out[2, 2:4]) == (320.0, 256.0)
    if name == "degenerate":
        assert rows[0, 0, 2] == 0.0 and rows[1, 0, 3] == 0.0


# ---- the public interface: refused by argument name before any device use ---------------------------------------------------------------
FRAME = np.full((96, 80, 3), 114, np.uint8)


@pytest.mark.parametrize("kwargs,word", [(dict(merge_metric="ios"), "merge_metric"), (dict(merge_mode="union"), "merge_mode"),
                                         (dict(merge_mode="wbf"), "merge_mode"), (dict(augment=True), "augment")])
def test_tile_refusals_for_obb_models_name_the_argument(kwargs, word):
    y = YOLO("yolov8n-obb.yaml")
    with pytest.raises(NotImplementedError, match=word):
        y.predict([FRAME], tile=64, **kwargs)
    assert y.predictor is None and all(p.device.type == "cpu" for p in y.model.parameters())


def test_tile_with_a_float_tensor_is_refused_first_for_obb_models():
    y = YOLO("yolov8n-obb.yaml")
    with pytest.raises(NotImplementedError, match=r"^tile.*uint8 pixels"):
        y.predict(torch.zeros(1, 3, 64, 64), tile=64)
    with pytest.raises(NotImplementedError, match="track"):
        y.track([FRAME], tile=64)
    assert y.predictor is None and all(p.device.type == "cpu" for p in y.model.parameters())


def test_obb_predictor_refuses_the_same_before_the_device():
    from drone_yolo_amd.engine.predictor import OBBPredictor

    y = YOLO("yolov8n-obb.yaml")
    for kwargs, word in ((dict(merge_metric="ios"), "merge_metric"), (dict(merge_mode="wbf"), "merge_mode"), (dict(augment=True), "augment")):
        with pytest.raises(NotImplementedError, match=word):
            OBBPredictor(y.model, dict(tile=64, **kwargs))
    with pytest.raises(ValueError, match="tile"):  # (the detection task's own check of the tile size stays in front of the device too)
        OBBPredictor(y.model, dict(tile=50))
    assert all(p.device.type == "cpu" for p in y.model.parameters())
