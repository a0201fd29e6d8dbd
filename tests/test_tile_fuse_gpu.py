"""GPU: the fusing cross-tile merge ``dy_tile_fuse`` (csrc/tile_merge.hip; ``H.tile_merge(..., mode="union" | "wbf")``) bit for bit against the
numpy restatement ``fuse_ref`` of tests/_fuse_util.py, its determinism, the untouched suppress path, then ``merge_mode=`` through YOLO.predict /
YOLO.track against the CPU oracle chain fused by ``fuse_ref``."""
import functools
import types

import numpy as np
import pytest
import torch

import drone_yolo_amd as D
from drone_yolo_amd import hip_ops as H
from oracle import drone_yolo_oracle as O
from tests._fuse_util import FUSE_SEEDS, SPLIT_FRAME, fuse_ref, split_rows
from tests._tile_util import CASES, IOS_THR, IOU_THR, MARGIN, SEEDS, block_frame, merge_margin, merge_ref, oracle_tile_chain, tile_rows
from tests._track_util import assert_rows_match
from tests._util import golden
from tests.test_model_gpu import _build

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _rows(name):
    return tile_rows(SEEDS[name], *CASES[name])


@functools.lru_cache(maxsize=None)
def _ref(name, metric, agnostic, keep, mode):
    rows, counts, offs = _rows(name)
    return fuse_ref(rows, counts, offs, CASES[name][4], IOS_THR if metric else IOU_THR, metric, agnostic, keep, mode)


def _device_rows(name, device):
    return tuple(torch.from_numpy(a).to(device) for a in _rows(name))


def _poisoned(F, K, md, keep, device):
    """Buffers of their own whose outputs hold values the kernel never writes."""
    b = H.TileMergeBuffers(F, K, md, keep, device, fuse=True)
    b.out.fill_(float("nan")), b.count.fill_(-7), b.index.fill_(-7), b.members.fill_(-7)
    return b


def _host(b):
    return b.out.cpu().numpy(), b.count.cpu().numpy(), b.index.cpu().numpy(), b.members.cpu().numpy()


def _assert_bit_equal(got, exp, what=""):
    (out, cnt, idx, mem), (eo, ec, ei, em) = got, exp
    assert np.array_equal(cnt, ec), (what, cnt, ec)
    assert np.array_equal(idx, ei), what  # the same slots in the same order, -1 beyond the count
    assert mem.dtype == np.int32 and np.array_equal(mem, em), what  # members >= 1 of every kept row, 0 beyond the count
    assert np.array_equal(out.view(np.uint32), eo.view(np.uint32)), what  # rows bit-equal, rows >= count zero


# (case, merge_max_det): one tile; the LDS sort with ragged counts and an empty frame; the same truncated in the middle of a chunk of 64 (rows
# behind the stop are absorbed or dropped); 12,000 slots per frame; the same at 4096 kept rows, which fills (rows are dropped) and whose kept
# list leaves LDS for 4,096 keys only: the keys are sorted in the workspace, where the wbf weights are then read from
FUSE_RUNS = [("one_tile", 1000), ("lds", 1000), ("lds", 16), ("4k", 1000), ("4k", 4096)]


@pytest.mark.parametrize("agnostic", [False, True], ids=["by_class", "agnostic"])
@pytest.mark.parametrize("metric", [0, 1], ids=["iou", "ios"])
@pytest.mark.parametrize("mode", ["union", "wbf"])
@pytest.mark.parametrize("name,keep", FUSE_RUNS, ids=[f"{n}-{k}" for n, k in FUSE_RUNS])
def test_tile_fuse_matches_numpy_restatement(device, name, keep, mode, metric, agnostic):
    F, K, md, nc, hw = CASES[name][:5]
    rows, counts, offs = _device_rows(name, device)
    bufs = _poisoned(F, K, md, keep, device)
    got = H.tile_merge((rows, counts), offs, K, hw, nc, IOS_THR if metric else IOU_THR, metric, agnostic, keep, bufs=bufs, mode=mode)
    assert got is bufs and (got.batch, got.max_det) == (F, keep) and got.members.shape == (F, keep)
    exp = _ref(name, metric, agnostic, keep, mode)
    _assert_bit_equal(_host(got), exp)
    if name != "one_tile":
        assert (exp[3] >= 2).any()  # something was absorbed
    if (name, keep) == ("lds", 16):
        assert (exp[1][[0, 2]] == 16).all() and exp[3][0].sum() < int(_rows(name)[1][:K].sum())  # truncated, and rows were dropped


def test_tile_fuse_workspace_sort_at_the_slot_limit(device):
    name, keep = "limit", 1000  # 32,700 slots: the keys are sorted in the workspace, beside the accumulators
    F, K, md, nc, hw = CASES[name][:5]
    rows, counts, offs = _device_rows(name, device)
    got = H.tile_merge((rows, counts), offs, K, hw, nc, IOS_THR, 1, False, keep, bufs=_poisoned(F, K, md, keep, device), mode="union")
    _assert_bit_equal(_host(got), _ref(name, 1, False, keep, "union"))


@pytest.mark.parametrize("mode", ["union", "wbf"])
def test_tile_fuse_two_launches_are_bit_identical(device, mode):
    name, keep = "4k", 1000
    F, K, md, nc, hw = CASES[name][:5]
    rows, counts, offs = _device_rows(name, device)
    bufs = _poisoned(F, K, md, keep, device)
    first = [a.copy() for a in _host(H.tile_merge((rows, counts), offs, K, hw, nc, IOU_THR, 0, False, keep, bufs=bufs, mode=mode))]
    second = _host(H.tile_merge((rows, counts), offs, K, hw, nc, IOU_THR, 0, False, keep, bufs=bufs, mode=mode))  # on the first launch's leftovers
    _assert_bit_equal(second, first)
    fresh = _host(H.tile_merge((rows, counts), offs, K, hw, nc, IOU_THR, 0, False, keep, bufs=_poisoned(F, K, md, keep, device), mode=H.TILE_MERGE_MODES[mode]))  # the mode by number
    _assert_bit_equal(fresh, first)


def test_tile_merge_mode_suppress_is_todays_call(device):
    name, keep = "lds", 1000
    F, K, md, nc, hw = CASES[name][:5]
    rows, counts, offs = _device_rows(name, device)
    plain = H.tile_merge((rows, counts), offs, K, hw, nc, IOS_THR, 1, False, keep)
    a = [t.clone() for t in (plain.out, plain.count, plain.index)]
    for mode in ("suppress", 0):
        named = H.tile_merge((rows, counts), offs, K, hw, nc, IOS_THR, 1, False, keep, mode=mode)
        assert named is plain  # the same persistent buffers
        assert all(torch.equal(x, y) for x, y in zip(a, (named.out, named.count, named.index)))
    eo, ec, ei = merge_ref(*_rows(name), hw, IOS_THR, 1, False, keep)
    assert np.array_equal(a[0].cpu().numpy().view(np.uint32), eo.view(np.uint32)) and np.array_equal(a[1].cpu().numpy(), ec) and np.array_equal(a[2].cpu().numpy(), ei)
    with pytest.raises(ValueError, match="mode"):
        H.tile_merge((rows, counts), offs, K, hw, nc, IOS_THR, 1, False, keep, mode="average")
    with pytest.raises(ValueError, match="mode"):
        H.tile_merge((rows, counts), offs, K, hw, nc, IOS_THR, 1, False, keep, mode=3)


def test_tile_fuse_split_object_no_tile_sees_whole(device):
    rows, counts, offs = (torch.from_numpy(a).to(device) for a in split_rows())
    sup = H.tile_merge((rows, counts), offs, 2, SPLIT_FRAME, 3, 0.8, "ios", False, 8)
    assert int(sup.count[0]) == 1 and sup.out[0, 0].tolist() == [46.0, 10.0, 64.0, 30.0, float(np.float32(0.9)), 1.0]  # the fragment
    got = H.tile_merge((rows, counts), offs, 2, SPLIT_FRAME, 3, 0.8, "ios", False, 8, bufs=_poisoned(1, 2, 4, 8, device), mode="union")
    out, cnt, idx, mem = _host(got)
    assert cnt[0] == 1 and idx[0].tolist() == [0] + [-1] * 7 and mem[0].tolist() == [2] + [0] * 7
    assert out[0, 0].tolist() == [46.0, 10.0, 100.0, 30.0, float(np.float32(0.9)), 1.0] and not out[0, 1:].any()  # the whole object
    _assert_bit_equal((out, cnt, idx, mem), fuse_ref(*split_rows(), SPLIT_FRAME, 0.8, 1, False, 8, "union"))
    got = H.tile_merge((rows, counts), offs, 2, SPLIT_FRAME, 3, 0.8, "ios", False, 8, bufs=_poisoned(1, 2, 4, 8, device), mode="wbf")
    _assert_bit_equal(_host(got), fuse_ref(*split_rows(), SPLIT_FRAME, 0.8, 1, False, 8, "wbf"))


# ---- merge_mode= through the public interface -------------------------------------------------------------------------------------------
TILE, OVERLAP, MERGE = 128, 0.25, 0.6
ARGS = dict(tile=TILE, tile_overlap=OVERLAP, merge_iou=MERGE, dtype="fp32", device=0)
SCORE_MARGIN = 1e-4  # (tests/test_tile_merge_gpu.py::_expected says why this is what the fixture allows)
METRICS = {"iou": 0, "ios": 1}
SHAPE = (200, 300)


@pytest.fixture(scope="module")
def chain(device):
    """The fixture model behind YOLO and, per frame, the CPU oracle's per-tile rows (computed once, shared, not modified)."""
    m, d, sd, model, _ = _build("n128", golden("e2e.npz"), device)
    yolo = D.YOLO(m["yaml"])
    yolo.model = model
    nc = m["nc"]

    @functools.lru_cache(maxsize=None)
    def oracle(seed):
        frame = block_frame(seed, SHAPE)
        rows, counts, offs, margins = oracle_tile_chain(O, d, sd, frame, TILE, OVERLAP, nc)
        return frame, rows, counts, offs, margins

    return types.SimpleNamespace(yolo=yolo, nc=nc, oracle=oracle)


def _expected(chain, seed, mode, metric):
    """The oracle's rows of one frame fused by fuse_ref, after asserting the two conditions the seed was chosen for (tests/_fuse_util.py):
    (a) the oracle keeps clear of every threshold of the chain, (b) fusion changes at least one row of the frame."""
    frame, rows, counts, offs, (m_conf, m_nms) = chain.oracle(seed)
    assert counts.sum() > 0 and m_conf >= SCORE_MARGIN, f"frame {seed}: an anchor's score within {SCORE_MARGIN} of conf ({m_conf})"
    assert m_nms >= MARGIN, f"frame {seed}: a same-class IoU within {MARGIN} of the per-tile NMS threshold"
    assert merge_margin(rows, counts, offs, MERGE, METRICS[metric]) >= MARGIN, f"frame {seed}: a same-class overlap within {MARGIN} of the merge threshold"
    so, sc, _ = merge_ref(rows, counts, offs, SHAPE, MERGE, METRICS[metric], False, 1000)
    out, cnt, _, mem = fuse_ref(rows, counts, offs, SHAPE, MERGE, METRICS[metric], False, 1000, mode)
    n = int(cnt[0])
    moved = np.abs(out[0, :n, :4] - so[0, :n, :4]).max(1)
    assert ((mem[0, :n] >= 2) & (moved > 0.5)).any(), f"frame {seed}: {mode} changes no row by more than half a pixel"
    return frame, out[0, :n]


def _assert_result(res, frame, exp, what):
    got = res.boxes.data.cpu().numpy()
    assert res.orig_shape == SHAPE and res.orig_img is frame, what
    assert got.shape == exp.shape, f"{what}: {got.shape[0]} rows, expected {exp.shape[0]}"
    assert np.array_equal(got[:, 5], exp[:, 5]), f"{what}: classes differ"
    assert np.allclose(got[:, :5], exp[:, :5], atol=3e-2, rtol=1e-4), f"{what}: boxes / scores differ by {np.abs(got[:, :5] - exp[:, :5]).max()}"


@pytest.mark.parametrize("mode,metric", list(FUSE_SEEDS), ids=[f"{m}-{k}" for m, k in FUSE_SEEDS])
def test_predict_tile_merge_mode_matches_oracle_chain(chain, mode, metric):
    exp = [_expected(chain, s, mode, metric) for s in FUSE_SEEDS[mode, metric]]
    frames = [e[0] for e in exp]
    kw = dict(merge_metric=metric, merge_mode=mode, **ARGS)
    streamed = chain.yolo.predict(frames, batch=2, stream=True, **kw)
    assert isinstance(streamed, types.GeneratorType)
    for what, res in (("one call", chain.yolo.predict(frames, **kw)), ("batch=2", chain.yolo.predict(frames, batch=2, **kw)), ("stream", list(streamed))):
        assert len(res) == len(frames)
        for i, (frame, rows) in enumerate(exp):
            _assert_result(res[i], frame, rows, f"{mode} / {metric}, {what}, frame {i}")
    sup = chain.yolo.predict(frames, merge_metric=metric, **ARGS)  # the default mode still suppresses: same rows, scores and classes, other boxes
    for i, (_, rows) in enumerate(exp):
        got = sup[i].boxes.data.cpu().numpy()
        assert got.shape == rows.shape and np.array_equal(got[:, 5], rows[:, 5]) and np.abs(got[:, :4] - rows[:, :4]).max() > 0.4


def test_track_tile_union_device_tracker_equals_host_tracker(chain):
    """The fused rows through the track step on the device and through the host tracker; persist=True goes on across two calls."""
    base = block_frame(FUSE_SEEDS["union", "ios"][0], SHAPE)
    frames = [np.ascontiguousarray(np.roll(base, (2 * f, 3 * f), (0, 1))) for f in range(6)]  # a short video: the frame drifting a few pixels per step
    targs = dict(conf=0.25, merge_mode="union", **ARGS)
    dev = chain.yolo.track(frames, batch=3, **targs)
    dev_a = chain.yolo.track(frames[:3], **targs)
    dev_b = chain.yolo.track(frames[3:], persist=True, **targs)
    host = chain.yolo.track(frames, batch=3, device_track=False, **targs)
    host_a = chain.yolo.track(frames[:3], device_track=False, **targs)
    host_b = chain.yolo.track(frames[3:], persist=True, device_track=False, **targs)
    assert len(dev) == len(host) == 6 and any(r.boxes.is_track for r in dev)
    det = chain.yolo.predict(frames, conf=0.25, merge_mode="union", **ARGS)
    sup = chain.yolo.predict(frames, conf=0.25, **ARGS)
    assert [len(r) for r in det] == [len(r) for r in sup]  # fusion keeps the rows suppression keeps ...
    assert any(not np.array_equal(a.boxes.data.cpu().numpy(), b.boxes.data.cpu().numpy()) for a, b in zip(det, sup))  # ... with other boxes
    for f in range(6):
        assert dev[f].orig_shape == SHAPE and dev[f].orig_img is frames[f]
        assert dev[f].boxes.is_track == host[f].boxes.is_track
        if dev[f].boxes.is_track:
            assert_rows_match(dev[f].boxes.data.cpu().numpy(), host[f].boxes.data.cpu().numpy(), f"frame {f}")
            assert len(dev[f]) <= len(det[f])  # tracks are made of the frame's fused rows
    for f, (d2, h2) in enumerate(zip(dev_a + dev_b, host_a + host_b)):
        assert d2.boxes.is_track == h2.boxes.is_track
        if d2.boxes.is_track:
            assert_rows_match(d2.boxes.data.cpu().numpy(), h2.boxes.data.cpu().numpy(), f"persist, frame {f}")
            assert np.array_equal(d2.boxes.data.cpu().numpy(), dev[f].boxes.data.cpu().numpy())  # two calls with persist = one call
