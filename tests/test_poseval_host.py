"""Pose validation without a GPU: ``kpt_iou``, ``PoseMetrics``, the host arithmetic of ``PoseValidator`` against the reference's recorded ``tp_p``,
the ``synthetic-pose`` dataset, the loader's ``keypoints``, the dataset refusals of ``YOLO.val``, the new entry point's argument checks, and the
conditions under which tests/golden/poseval.npz's cases were accepted (tools/make_poseval_golden.py), re-derived here from the stored seeds with
this package's restatements of ``kpt_iou`` and ``match_predictions``."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from drone_yolo_amd import YOLO
from drone_yolo_amd.engine.trainer import TensorLoader, load_dataset
from drone_yolo_amd.engine.validator import PoseValidator, pose_label_kpts
from drone_yolo_amd.utils.metrics import OKS_SIGMA, DetMetrics, PoseMetrics, box_iou, kpt_iou, match_predictions
from tests import _poseval_util as V
from tests._util import golden, meta

MATCH_NAMES = list(V.MATCH_CASES) + ["single_cls"]


@pytest.fixture(scope="module")
def g():
    return golden("poseval.npz")


def _oks32(tbox, tkpt, pk, sigma):
    tb = torch.from_numpy(np.ascontiguousarray(tbox, dtype=np.float32))
    area = ((tb[:, 2] - tb[:, 0]) * (tb[:, 3] - tb[:, 1])) * 0.53
    return kpt_iou(np.ascontiguousarray(tkpt, dtype=np.float32), np.ascontiguousarray(pk, dtype=np.float32), area, sigma).numpy()


def _match32(pcls, tcls, iou):
    return match_predictions(np.asarray(pcls, np.float32), np.asarray(tcls, np.float32), np.asarray(iou, np.float32), V.IOUV)


def unpack(g, key, shape):
    return np.unpackbits(g[key])[: int(np.prod(shape))].reshape(shape).astype(bool)


@functools.lru_cache(maxsize=None)
def match_case(name):
    """(inputs, float64 / fp32 evaluation) of a kernel-free case at its stored seed: computed once, shared, not modified."""
    g = golden("poseval.npz")
    c = V.match_inputs(name, int(g[f"m_{name}__seed"]))
    return c, V.match_evaluate(c, _oks32, _match32, fixed=float(g[f"m_{name}__margin"][0]))


def _same_class_scores(c, e):
    out, k = [], 0
    for i, cnt in enumerate(c["counts"]):
        where = np.nonzero(c["timg"] == i)[0]
        if cnt == 0 or len(where) == 0:
            continue
        pcls = np.zeros(cnt, np.float32) if c["single_cls"] else c["rows"][i, :cnt, 5]
        out.append(e["oks32"][k][c["tcls"][where][:, None] == pcls[None]])
        k += 1
    return np.concatenate(out)


def test_posemetrics_carries_the_reference_keys_and_sigma():
    m = PoseMetrics()
    assert m.keys == DetMetrics.keys + ("metrics/precision(P)", "metrics/recall(P)", "metrics/mAP50(P)", "metrics/mAP50-95(P)")
    assert list(m.results_dict) == list(m.keys) + ["fitness"] and all(v == 0.0 for v in m.results_dict.values())
    assert OKS_SIGMA.shape == (17,) and np.array_equal(OKS_SIGMA, V.COCO_SIGMA)
    v = PoseValidator(dict(conf=None, iou=0.6, max_det=50, single_cls=True))
    assert isinstance(v.metrics, PoseMetrics) and v.stat_keys == ("tp", "tp_p") and not v.val_loss and v.conf == 0.001 and v.device_match and v.last_stats is None


@pytest.mark.parametrize("name", MATCH_NAMES)
def test_match_fixture_conditions_hold_at_the_stored_seed(g, name):
    c, e = match_case(name)
    B, md = len(c["counts"]), c["max_det"]
    assert e["ok"], f"{name}: the acceptance conditions do not hold at seed {int(g[f'm_{name}__seed'])}"
    M, floor = float(g[f"m_{name}__margin"][0]), float(g["m_val300__margin"][0])
    # (judged with the recorded margin; what this CPU's fp32 measures stays within a factor of two of it)
    assert e["M_meas"] <= 2 * M and M >= floor and (name != "val300" or e["M_meas"] >= M / 2)
    assert 0 < M < 1e-4
    rec = unpack(g, f"m_{name}__tp", (B, md, 10))
    assert np.array_equal(rec, e["tp32"]) and np.array_equal(rec, e["tp64"]) and rec.any()
    assert np.array_equal(g[f"m_{name}__best_label"], e["best_label64"]) and np.allclose(g[f"m_{name}__best_iou"], e["best_iou64"], rtol=0, atol=1e-12)
    for i, cnt in enumerate(c["counts"]):
        assert not rec[i, cnt:].any()


@pytest.mark.parametrize("name", MATCH_NAMES)
def test_kpt_iou_against_the_recorded_fp32_oks(g, name):
    """``utils.metrics.kpt_iou`` on the same fp32 inputs against the reference's own fp32 scores of every same-class pair: the same operations in the
    same order, so at most the last bits of this CPU's exp and sum differ (a quarter of the recorded margin = 2 x the measured fp32 error)."""
    c, e = match_case(name)
    rec, got = g[f"m_{name}__oks32"], _same_class_scores(c, e)
    assert rec.dtype == np.float32 and rec.shape == got.shape and len(rec)
    worst = float(np.abs(got - rec.astype(np.float64)).max())
    print(f"kpt_iou {name}: max |this package - the reference's fp32| {worst:.3e} over {len(rec)} pairs")
    assert worst <= float(g[f"m_{name}__margin"][0]) / 4


def test_match_cases_are_what_they_are_for(g):
    c, e = match_case("val300")
    assert c["counts"].tolist() == [300, 37] and np.bincount(c["timg"]).tolist() == [40, 12] and len(np.unique(c["tcls"])) == 3
    c, e = match_case("few")
    assert c["counts"].tolist() == [0, 1, 5] and np.bincount(c["timg"], minlength=3).tolist() == [3, 0, 4] and not np.all(np.diff(c["timg"]) >= 0)
    c, e = match_case("rank")  # the higher-ranked detection has the lower OKS and the same best label
    b0, b1 = e["best_iou64"][0, :2]
    assert e["best_label64"][0, 0] == e["best_label64"][0, 1] == 0 and 0.5 < b0 < b1
    both = V.IOUV <= b0
    assert both.sum() >= 2 and (V.IOUV[~both] <= b1).sum() >= 2
    assert e["tp64"][0, 0].tolist() == both.tolist(), "the higher-ranked detection takes the label at the thresholds it reaches"
    assert e["tp64"][0, 1].tolist() == (~both & (V.IOUV <= b1)).tolist(), "the later one loses it there and wins it at the thresholds only it reaches"
    c, e = match_case("step")
    assert len(c["tbox"]) == 130 > V.STAGE and c["max_det"] == 16 and np.bincount(c["timg"]).tolist() == [80, 50]
    c, e = match_case("stride")
    assert c["counts"].tolist() == [520, 3] and c["max_det"] == 520 > V.THREADS
    c, e = match_case("clip")
    W, H = c["clip"]
    pk = c["kpts"][0, : c["counts"][0]]
    assert (pk[..., 0] < 0).any() or (pk[..., 0] > W).any() or (pk[..., 1] < 0).any() or (pk[..., 1] > H).any()
    assert (c["tkpt"][..., 0] == 0).any() and (c["tkpt"][..., 1] == H).any() and (c["tkpt"][..., 0] == W).any() and (c["tkpt"][..., 1] == 0).any()
    c, e = match_case("invisible")
    nvis = (c["tkpt"][..., 2] != 0).sum(1)
    assert (nvis == 0).sum() == 1 and (nvis == 1).sum() >= 1 and set(np.unique(c["tkpt"][..., 2])) == {0.0, 1.0, 2.0}
    blind = int(np.flatnonzero(nvis == 0)[0])
    cnt = c["counts"][c["timg"][blind]]
    assert not (e["tp64"][c["timg"][blind], :cnt].any(1) & (e["best_label64"][c["timg"][blind], :cnt] == blind)).any(), "a label without a visible keypoint is never matched"
    c, e = match_case("zero_area")
    assert ((c["tbox"][:, 2] - c["tbox"][:, 0]) == 0).sum() == 1
    c, e = match_case("kpt4x2")
    assert c["kpt_shape"] == (4, 2) and c["kpts"].shape[2:] == (4, 2) and np.array_equal(V.sigma_of((4, 2)), np.full(4, 0.25))
    c, e = match_case("single_cls")
    assert c["single_cls"] and not c["tcls"].any() and e["tp64"].any() and np.array_equal(c["kpts"], match_case("few")[0]["kpts"])


@functools.lru_cache(maxsize=None)
def seedless_case(name):
    """(inputs, float64 tp, float64 best label) of the full-stage / layout-bound cases: computed once, shared, not modified."""
    c = dict(full_stage=V.full_stage_case, bound=V.bound_case)[name]()
    tp, best, scores = V.expect64(c)
    assert ((scores > 0.999) | (scores < 1e-6)).all(), "every threshold is decided by a margin thousands of times the recorded M"
    return c, tp, best


def test_full_stage_and_bound_cases_are_what_they_are_for():
    c, tp, best = seedless_case("full_stage")
    assert len(c["tbox"]) == V.STAGE + 1 and not c["timg"].any() and (c["tcls"] == 1).all() and c["counts"].tolist() == [4] and c["max_det"] == 4
    assert best.tolist() == [0, V.STAGE - 1, V.STAGE, V.STAGE] and tp[:3].all() and not tp[3].any()
    c, tp, best = seedless_case("bound")
    assert c["max_det"] == 4096 and c["counts"].tolist() == [4096] and c["kpt_shape"] == (32, 2) and not np.isin(c["rows"][0, 5:, 5], c["tcls"]).any()
    assert best[:5].tolist() == [0, 1, 2, 3, 4] and tp[:5].all() and not tp[5:].any()


# ---- the validator's host arithmetic on the recorded rows ------------------------------------------------------------------------------
def e2e_fixture(g, tag):
    m = meta(g, tag)
    n = m["shape"][0]
    nkpt, ndim = m["kpt_shape"]
    counts = g[f"{tag}__counts"]
    cm = g[f"{tag}__rows"].shape[1]
    rows, kpts = np.zeros((n, 300, 6), np.float32), np.zeros((n, 300, nkpt, ndim), np.float32)
    rows[:, :cm], kpts[:, :cm] = g[f"{tag}__rows"], g[f"{tag}__kpts"]
    return (m, counts, rows, kpts, unpack(g, f"{tag}__tp", (n, 300, 10)), unpack(g, f"{tag}__tp_p", (n, 300, 10)),
            dict(zip((str(k) for k in g[f"{tag}__result_keys"]), g[f"{tag}__results"])))


@pytest.mark.parametrize("tag", list(V.E2E))
def test_host_match_on_recorded_rows_gives_the_reference_tp_and_dict(g, tag):
    m, counts, rows, kpts, tp_ref, tpp_ref, res_ref = e2e_fixture(g, tag)
    h, w = m["shape"][2:]
    sigma = V.sigma_of(m["kpt_shape"])
    bidx, cls, bboxes, lk = g[f"{tag}__batch_idx"], g[f"{tag}__cls"], torch.from_numpy(g[f"{tag}__bboxes"]), torch.from_numpy(g[f"{tag}__keypoints"])
    assert lk.shape[1:] == tuple(m["kpt_shape"][:1]) + (3,) and all((bidx == i).any() for i in range(len(counts))), "every image has labels"
    assert set(np.unique(g[f"{tag}__keypoints"][..., 2])) == {0.0, 1.0, 2.0}
    v = PoseValidator(dict(conf=m["conf"], iou=m["iou"]))
    lim = torch.tensor((w, h, w, h), dtype=torch.float32)
    stats = dict(tp=[], tp_p=[], conf=[], pred_cls=[], target_cls=[])
    scores = []
    for i, k in enumerate(counts):
        sel = bidx == i
        tbox = v._labels(bboxes[sel], w, h, lim).numpy()
        tkpt = pose_label_kpts(lk[sel], w, h, lim).numpy()
        pn = v._clipped(rows[i, :k], w, h)
        oks = _oks32(tbox, tkpt, V.clip_kpts(kpts[i, :k], w, h), sigma)
        tp, tp_p = match_predictions(pn[:, 5], cls[sel], box_iou(tbox, pn[:, :4]), v.iouv), match_predictions(pn[:, 5], cls[sel], oks, v.iouv)
        assert np.array_equal(tp, tp_ref[i, :k]) and np.array_equal(tp_p, tpp_ref[i, :k]), f"{tag}: image {i}"
        scores.append(oks[cls[sel][:, None] == pn[None, :, 5]])
        for key, val in (("tp", tp), ("tp_p", tp_p), ("conf", pn[:, 4]), ("pred_cls", pn[:, 5]), ("target_cls", cls[sel])):
            stats[key].append(val)
    scores = np.concatenate(scores)
    assert scores.min() < 0.5 and scores.max() > 0.95, "the labels' OKS runs from below 0.5 to nearly 1"
    near = np.abs(scores.astype(np.float64)[:, None] - V.IOUV[None]).min()
    assert near >= m["near"] - 2 * m["margin"] > 2e-4, "no same-class pair near a threshold"
    v.metrics.process(*(np.concatenate(stats[k]) for k in ("tp", "tp_p", "conf", "pred_cls", "target_cls")))
    got = v.metrics.results_dict
    assert set(got) == set(res_ref)
    for k in got:
        assert round(float(got[k]), 5) == round(float(res_ref[k]), 5), (k, got[k], res_ref[k])
    assert tpp_ref.any() and tp_ref.any() and res_ref["metrics/mAP50(P)"] > 0
    assert float(m["margin"]) >= float(g["m_val300__margin"][0])


# ---- data -------------------------------------------------------------------------------------------------------------------------------
def test_synthetic_pose_adds_keypoints_behind_the_same_draws():
    for kpt_shape in ((17, 3), (4, 2)):
        d, base = load_dataset("synthetic-pose:5", 64, 3, 2, kpt_shape=kpt_shape), load_dataset("synthetic:5", 64, 3, 2)
        assert set(d) == set(base) | {"keypoints"} and all(torch.equal(d[k], base[k]) for k in base), "the box, class and image draws equal 'synthetic:N''s"
        k, b = d["keypoints"], d["bboxes"]
        assert tuple(k.shape) == (b.shape[0], kpt_shape[0], 3) and k.dtype == torch.float32
        assert set(k[..., 2].unique().tolist()) == {0.0, 1.0, 2.0} and bool(((k[..., 2] != 0).sum(1) >= 1).all()), "at least one visible point per label"
        lo, hi = (b[:, :2] - b[:, 2:] / 2)[:, None], (b[:, :2] + b[:, 2:] / 2)[:, None]
        assert bool(((k[..., :2] >= lo - 1e-6) & (k[..., :2] <= hi + 1e-6)).all()), "every point lies inside its box"
    with pytest.raises(NotImplementedError, match="kpt_shape"):
        load_dataset("synthetic-pose:5", 64, 3, 2)


def test_loader_yields_the_label_rows_keypoints_in_label_order_at_a_ragged_batch():
    kp = torch.arange(5 * 4 * 3, dtype=torch.float32).view(5, 4, 3)
    data = dict(img=torch.zeros((3, 3, 32, 32), dtype=torch.uint8), batch_idx=torch.tensor([2.0, 0.0, 2.0, 1.0, 0.0]), cls=torch.zeros((5, 1)),
                bboxes=torch.rand(5, 4), keypoints=kp)
    batches = list(TensorLoader(load_dataset(data, 32, 3, 0), 2, 0, 1, shuffle=False))
    assert [tuple(b["keypoints"].shape) for b in batches] == [(3, 4, 3), (2, 4, 3)]
    assert torch.equal(batches[0]["keypoints"], kp[[1, 4, 3]]) and torch.equal(batches[0]["bboxes"], data["bboxes"][[1, 4, 3]]) and batches[0]["batch_idx"].tolist() == [0.0, 0.0, 1.0]
    assert torch.equal(batches[1]["keypoints"], kp[[0, 2]]) and batches[1]["batch_idx"].tolist() == [0.0, 0.0]
    plain = {k: v for k, v in data.items() if k != "keypoints"}
    assert "keypoints" not in next(iter(TensorLoader(plain, 2, 0, 1, shuffle=False)))


def test_pose_label_kpts_scales_clips_and_appends_the_visibility():
    k = torch.tensor([[[0.5, 0.25, 2.0], [-0.1, 1.2, 0.0], [1.5, -0.3, 1.0]]])
    lim = torch.tensor((96.0, 64.0, 96.0, 64.0))
    out = pose_label_kpts(k, 96, 64, lim)
    assert out.tolist() == [[[48.0, 16.0, 2.0], [0.0, 64.0, 0.0], [96.0, 0.0, 1.0]]]
    assert pose_label_kpts(k[..., :2], 96, 64, lim).tolist() == [[[48.0, 16.0, 1.0], [0.0, 64.0, 1.0], [96.0, 0.0, 1.0]]], "two columns mean all visible"


# ---- YOLO.val ---------------------------------------------------------------------------------------------------------------------------
def test_val_refuses_a_dataset_without_matching_keypoints_before_any_device_use():
    y = YOLO("yolov8n-pose.yaml")
    data = dict(img=torch.zeros((2, 3, 64, 64), dtype=torch.uint8), batch_idx=torch.tensor([0.0, 1.0]), cls=torch.zeros((2, 1)),
                bboxes=torch.tensor([[0.5, 0.5, 0.2, 0.2], [0.4, 0.4, 0.1, 0.3]]))
    for d in (data, "synthetic:4"):
        with pytest.raises(NotImplementedError, match=r"val: a pose model needs a dataset with 'keypoints'.*has none"):
            y.val(data=d, device=0)
    for bad in (torch.zeros(2, 5, 3), torch.zeros(2, 17, 2), torch.zeros(3, 17, 3), torch.zeros(2, 51)):  # nkpt, all-visible form under ndim 3, rows, rank
        with pytest.raises(NotImplementedError, match=r"val: a pose model needs a dataset with 'keypoints'.*kpt_shape \[17, 3\]"):
            y.val(data=dict(data, keypoints=bad), device=0)
    assert y.predictor is None and getattr(y, "metrics", None) is None
    assert all(p.device.type == "cpu" for p in y.model.parameters())
    with pytest.raises(NotImplementedError, match="train"):
        y.train(data="synthetic-pose:4")
    with pytest.raises(ValueError, match="data"):
        y.val()


# ---- the C interface without a device -------------------------------------------------------------------------------------------------
def test_new_entry_point_validates_without_gpu(tmp_path):
    import os
    import subprocess

    from drone_yolo_amd import _lib as L
    from tests._util import ROOT

    h = L.lib()
    m = L.ValOksMatchDesc()
    assert h.dy_val_oks_match(ctypes.byref(m), None) == -1 and b"dy_val_oks_match" in h.dy_last_error_string()
    assert h.dy_val_oks_match(None, None) == -1
    buf = ctypes.cast((ctypes.c_float * 64)(), ctypes.c_void_p)
    thr = (ctypes.c_float * 10)(*V.IOUV.tolist())
    sg = (ctypes.c_float * 64)(*([0.05] * 64))
    m.rows = m.counts = m.kpts = m.tp = buf
    m.sigma, m.iouv, m.batch, m.max_det, m.n_iouv, m.nkpt, m.ndim = sg, thr, 1, 4097, 10, 17, 3
    m.stride_b, m.stride_ch, m.stride_d = 300 * 51, 1, 51
    assert h.dy_val_oks_match(ctypes.byref(m), None) == -1 and b"max_det" in h.dy_last_error_string()
    m.max_det = 0
    assert h.dy_val_oks_match(ctypes.byref(m), None) == -1 and b"max_det" in h.dy_last_error_string()
    m.max_det, m.n_iouv = 300, 17
    assert h.dy_val_oks_match(ctypes.byref(m), None) == -1 and b"n_iouv" in h.dy_last_error_string()
    m.n_iouv, m.ndim = 10, 4
    assert h.dy_val_oks_match(ctypes.byref(m), None) == -1 and b"ndim" in h.dy_last_error_string()
    m.ndim, m.nkpt = 3, L.OKS_MAX_KPT + 1
    assert h.dy_val_oks_match(ctypes.byref(m), None) == -2 and b"nkpt" in h.dy_last_error_string()  # DY_ERR_UNSUPPORTED
    m.nkpt, m.n_labels = 17, 3
    assert h.dy_val_oks_match(ctypes.byref(m), None) == -1 and b"label pointer" in h.dy_last_error_string()
    m.tbox = m.tkpt = m.tcls = m.timg = ctypes.c_void_p(buf.value + 4)
    assert h.dy_val_oks_match(ctypes.byref(m), None) == -1 and b"16-byte" in h.dy_last_error_string()
    assert L.OKS_MAX_KPT >= 17
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include "dyolo.h"\nint main(){printf("%zu %d\\n", sizeof(dy_val_oks_match_desc), DY_OKS_MAX_KPT);return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "s")])
    assert [int(v) for v in subprocess.check_output([str(tmp_path / "s")]).split()] == [ctypes.sizeof(L.ValOksMatchDesc), L.OKS_MAX_KPT]
