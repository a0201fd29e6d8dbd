"""``dy_val_match`` (csrc/val_match.hip) and the validator's ``device_match`` data flow.

a. the kernel against the host functions it replaces (``utils.metrics.box_iou`` + ``match_predictions``) on one batch of five images with
   unsorted labels: ``tp`` equal, ``best_iou`` BIT-equal, ``best_label`` the argmax.  The inputs and the host's answers need no GPU:
   ``test_batch_case_is_as_intended`` checks on the CPU that the case has no exact tie for first place at or above 0.5.
b. hand-made images whose rows were evaluated with the host function (inclusive thresholds compared in fp32, label contention),
   ``single_cls``, no labels, one threshold, and a captured launch replayed on new rows.
c. ``DetectionValidator`` / ``YOLO.val`` with ``device_match``: the same dict as the host path, through the device path (call counts)."""
import functools

import numpy as np
import pytest
import torch

from drone_yolo_amd import hip_ops as H
from drone_yolo_amd.utils.metrics import box_iou, match_predictions

IOUV = np.linspace(0.5, 0.95, 10)
MAX_DET, CLIP_W, CLIP_H, NC = 300, 640, 512, 3
COUNTS, NLAB = (0, 1, 37, 300, 299), (3, 0, 40, 700, 1)


# more detections than the workgroup has threads (a thread runs several) and more than two rounds of them; labels beyond one step
WIDE_COUNTS, WIDE_NLAB, WIDE_MAX_DET = (1100, 5, 513), (600, 30, 513), 1100


@functools.lru_cache(maxsize=None)
def batch_case(seed=11, COUNTS=COUNTS, NLAB=NLAB, MAX_DET=MAX_DET):
    """rows (images, max_det, 6), counts, shuffled labels (tbox, tcls, timg) and the host's tp / best_iou / best_label for them."""
    rng = np.random.default_rng(seed)
    tbox, tcls, timg = [], [], []
    rows = (rng.standard_normal((len(COUNTS), MAX_DET, 6)) * 1e3).astype(np.float32)  # garbage beyond the counts
    for i, (cnt, nl) in enumerate(zip(COUNTS, NLAB)):
        wh = rng.uniform(8, 80, (nl, 2))
        c = rng.uniform(0, 1, (nl, 2)) * (np.array([CLIP_W, CLIP_H]) - wh) + wh / 2
        lb = np.concatenate((c - wh / 2, c + wh / 2), 1).astype(np.float32).clip(0, [CLIP_W, CLIP_H, CLIP_W, CLIP_H]).astype(np.float32)
        lc = rng.integers(0, NC, nl).astype(np.float32)
        tbox.append(lb), tcls.append(lc), timg.append(np.full(nl, i))
        if cnt == 0:
            continue
        if nl:
            src = rng.integers(0, nl, cnt)
            pb = lb[src] + rng.normal(0, 3, (cnt, 4))  # jittered copies of labels
            pc = lc[src].copy()
            flip = rng.random(cnt) < 0.2
            pc[flip] = (pc[flip] + rng.integers(1, NC, flip.sum())) % NC
            out = rng.random(cnt) < 0.06  # a few stick out of the image: the clip matters
            pb[out, 2] += CLIP_W - pb[out, 2] + rng.uniform(1, 30, out.sum())
            out = rng.random(cnt) < 0.06
            pb[out, 1] -= pb[out, 1] + rng.uniform(1, 30, out.sum())
        else:
            pb = np.concatenate((rng.uniform(0, 300, (cnt, 2)), rng.uniform(300, 500, (cnt, 2))), 1)
            pc = rng.integers(0, NC, cnt).astype(np.float32)
        rows[i, :cnt, :4] = pb
        rows[i, :cnt, 4] = np.sort(rng.uniform(0.001, 1, cnt))[::-1]
        rows[i, :cnt, 5] = pc
    tbox, tcls, timg = np.concatenate(tbox), np.concatenate(tcls), np.concatenate(timg)
    perm = rng.permutation(len(tbox))  # batch layout: labels belong to images by value, in no order
    tbox, tcls, timg = tbox[perm], tcls[perm], timg[perm]
    return dict(rows=rows, counts=np.array(COUNTS, np.int32), tbox=tbox, tcls=tcls, timg=timg, **host_expect(rows, COUNTS, tbox, tcls, timg))


def host_expect(rows, counts, tbox, tcls, timg, clip=(CLIP_W, CLIP_H)):
    """The host's tp / best_iou / best_label (``box_iou`` + ``match_predictions`` on the clipped rows) and the class-masked IoU of every image."""
    n, max_det = rows.shape[:2]
    exp_tp = np.zeros((n, max_det, len(IOUV)), bool)
    exp_iou = np.zeros((n, max_det), np.float32)
    exp_lab = np.full((n, max_det), -1, np.int64)
    masked = []
    for i, cnt in enumerate(counts):
        where = np.nonzero(timg == i)[0]
        if cnt == 0 or len(where) == 0:
            continue
        pn = rows[i, :cnt].copy()
        pn[:, [0, 2]] = pn[:, [0, 2]].clip(0, clip[0])
        pn[:, [1, 3]] = pn[:, [1, 3]].clip(0, clip[1])
        iou = box_iou(tbox[where], pn[:, :4])
        exp_tp[i, :cnt] = match_predictions(pn[:, 5], tcls[where], iou, IOUV)
        m = iou * (tcls[where][:, None] == pn[:, 5])
        assert m.dtype == np.float32
        exp_iou[i, :cnt] = m.max(0)
        exp_lab[i, :cnt] = where[m.argmax(0)]
        masked.append(m)
    return dict(tp=exp_tp, best_iou=exp_iou, best_label=exp_lab, masked=masked)


@functools.lru_cache(maxsize=None)
def full_stage_case():
    """A stage filled exactly to capacity: 513 labels of one class, all of image 0 and in order (the first step stages 512 entries, the second
    one), disjoint 8 x 8 squares on a grid; detections = exact copies of labels 0, 511 and 512."""
    l = np.arange(513)
    x, y = 4.0 + 12.0 * (l % 23), 4.0 + 12.0 * (l // 23)
    tbox = np.stack((x, y, x + 8, y + 8), 1).astype(np.float32)
    rows = np.full((1, 4, 6), 7e5, np.float32)
    rows[0, :3, :4], rows[0, :3, 4], rows[0, :3, 5] = tbox[[0, 511, 512]], (0.9, 0.8, 0.7), 1.0
    c = dict(rows=rows, counts=np.array([3], np.int32), tbox=tbox, tcls=np.ones(513, np.float32), timg=np.zeros(513, np.int64))
    return dict(c, **host_expect(rows, c["counts"], tbox, c["tcls"], c["timg"]))


@functools.lru_cache(maxsize=None)
def bound_case():
    """The LDS layout at its upper bound: max_det 4096 (32 bytes per detection), all rows kept, 5 labels.  The first five detections are
    copies of the labels, the rest far-away boxes of a class no label has."""
    rng = np.random.default_rng(0)
    x = 10.0 + 40.0 * np.arange(5)
    tbox = np.stack((x, np.full(5, 10.0), x + 30, np.full(5, 40.0)), 1).astype(np.float32)
    tcls = np.array([0, 1, 0, 1, 2], np.float32)
    rows = np.zeros((1, 4096, 6), np.float32)
    rows[0, :, :4] = np.concatenate((rng.uniform(300, 400, (4096, 2)), rng.uniform(420, 500, (4096, 2))), 1)
    rows[0, :, 4], rows[0, :, 5] = np.linspace(0.99, 0.01, 4096), 7.0
    rows[0, :5, :4], rows[0, :5, 5] = tbox, tcls
    c = dict(rows=rows, counts=np.array([4096], np.int32), tbox=tbox, tcls=tcls, timg=np.zeros(5, np.int64))
    return dict(c, **host_expect(rows, c["counts"], tbox, tcls, c["timg"]))


def test_batch_case_is_as_intended():
    c = batch_case()
    assert not np.all(np.diff(c["timg"]) >= 0), "the labels are meant to be unsorted"
    assert np.bincount(c["timg"], minlength=5).tolist() == list(NLAB)
    assert c["tp"].any(axis=(1, 2)).tolist() == [False, False, True, True, True]
    assert 0.3 < c["tp"][3, :, 0].mean() < 1.0 and c["tp"][3, :, 9].sum() < c["tp"][3, :, 0].sum()  # matches, contention and misses
    assert (c["rows"][:, :, :4].max() > CLIP_W) and (c["rows"][3, :300, 1].min() < 0)
    wide = batch_case(12, WIDE_COUNTS, WIDE_NLAB, WIDE_MAX_DET)
    assert wide["tp"].any(axis=(1, 2)).all() and np.bincount(wide["timg"]).tolist() == list(WIDE_NLAB)
    for m in c["masked"] + wide["masked"]:  # no exact tie for first place at or above 0.5: there the reference's order is not defined
        if m.shape[0] > 1:
            top2 = np.sort(m, 0)[-2:]
            assert not ((top2[1] >= 0.5) & (top2[0] == top2[1])).any()


def test_full_stage_and_bound_cases_are_as_intended():
    c = full_stage_case()
    assert len(c["tbox"]) == 513 and not c["timg"].any() and (c["masked"][0] == 1).sum() == 3  # disjoint squares: one label per detection
    assert c["best_label"][0].tolist() == [0, 511, 512, -1] and c["tp"][0, :3].all() and (c["best_iou"][0, :3] == 1).all()
    c = bound_case()
    assert c["rows"].shape == (1, 4096, 6) and not np.isin(c["rows"][0, 5:, 5], c["tcls"]).any()
    assert c["tp"][0, :5].all() and not c["tp"][0, 5:].any() and c["best_label"][0, :5].tolist() == [0, 1, 2, 3, 4] and not c["best_iou"][0, 5:].any()


def nms_buffers(rows, counts, device):
    rows = torch.as_tensor(rows, dtype=torch.float32)
    bufs = H.NmsBuffers(rows.shape[0], 1, rows.shape[1], device)
    bufs.out.copy_(rows)
    bufs.count.copy_(torch.as_tensor(counts, dtype=torch.int32))
    return bufs


def run(device, rows, counts, tbox, tcls, timg, iouv=IOUV, clip=(CLIP_W, CLIP_H), single_cls=False):
    bufs = nms_buffers(rows, counts, device)
    lab = [torch.as_tensor(np.asarray(v)).to(device) for v in (np.asarray(tbox, np.float32).reshape(-1, 4), tcls, timg)]
    tp, bi, bl = H.val_match(bufs, lab[0], lab[1], lab[2], iouv, clip, single_cls=single_cls, want_best=True)
    assert H.last_kernel_name() == "val_match_kernel"
    return tp.cpu().numpy(), bi.cpu().numpy(), bl.cpu().numpy()


@pytest.mark.gpu
def test_kernel_equals_host_match_on_a_batch(device):
    c = batch_case()
    tp, bi, bl = run(device, c["rows"], c["counts"], c["tbox"], c["tcls"], c["timg"].astype(np.float32))  # (image indices as the loader gives them: float)
    assert tp.dtype == np.uint8 and tp.shape == (5, MAX_DET, 10)
    for i, cnt in enumerate(COUNTS):
        assert np.array_equal(tp[i, :cnt].astype(bool), c["tp"][i, :cnt]), f"image {i}: {(tp[i, :cnt].astype(bool) != c['tp'][i, :cnt]).sum()} cells differ"
        assert not tp[i, cnt:].any() and not bi[i, cnt:].any() and (bl[i, cnt:] == -1).all()
    assert np.array_equal(bi.view(np.uint32), c["best_iou"].view(np.uint32)), "best_iou is not bit-equal to the host's masked IoU maximum"
    assert np.array_equal(bl, c["best_label"])


@pytest.mark.gpu
def test_kernel_with_more_detections_than_threads(device):
    c = batch_case(12, WIDE_COUNTS, WIDE_NLAB, WIDE_MAX_DET)
    tp, bi, bl = run(device, c["rows"], c["counts"], c["tbox"], c["tcls"], c["timg"])
    for i, cnt in enumerate(WIDE_COUNTS):
        assert np.array_equal(tp[i, :cnt].astype(bool), c["tp"][i, :cnt]), f"image {i}"
        assert not tp[i, cnt:].any() and not bi[i, cnt:].any() and (bl[i, cnt:] == -1).all()
    assert np.array_equal(bi.view(np.uint32), c["best_iou"].view(np.uint32)) and np.array_equal(bl, c["best_label"])


@pytest.mark.gpu
def test_kernel_with_a_stage_filled_to_capacity(device):
    c = full_stage_case()
    tp, bi, bl = run(device, c["rows"], c["counts"], c["tbox"], c["tcls"], c["timg"])
    assert bl[0].tolist() == [0, 511, 512, -1] and np.array_equal(bl, c["best_label"])
    assert np.array_equal(bi.view(np.uint32), c["best_iou"].view(np.uint32)), "best_iou is not bit-equal to the host's"
    assert np.array_equal(tp.astype(bool), c["tp"]) and tp[0, :3].all() and not tp[0, 3].any()


@pytest.mark.gpu
def test_kernel_with_the_lds_layout_at_its_bound(device):
    c = bound_case()
    tp, bi, bl = run(device, c["rows"], c["counts"], c["tbox"], c["tcls"], c["timg"])
    assert tp.shape == (1, 4096, 10) and np.array_equal(tp.astype(bool), c["tp"]) and tp[0, :5].all() and not tp[0, 5:].any()
    assert np.array_equal(bi.view(np.uint32), c["best_iou"].view(np.uint32)) and not bi[0, 5:].any()
    assert np.array_equal(bl, c["best_label"]) and bl[0, :5].tolist() == [0, 1, 2, 3, 4]


def rows_of(tp):
    return ["".join(str(int(v)) for v in r) for r in tp]


def pred_rows(boxes, classes, max_det):
    r = np.full((1, max_det, 6), 7e5, np.float32)
    for d, (b, c) in enumerate(zip(boxes, classes)):
        r[0, d] = (*b, 0.9 - 0.1 * d, c)
    return r


@pytest.mark.gpu
def test_hand_made_images(device):
    # IoU exactly 0.5, 0.75, 1.0 and a wrong class: >= is inclusive and the thresholds are compared as fp32
    labels, lcls = [(0, 0, 200, 100), (300, 0, 700, 100), (0, 300, 100, 400)], [0, 0, 1]
    preds, pcls = [(0, 0, 100, 100), (300, 0, 600, 100), (0, 300, 100, 400), (0, 300, 100, 400)], [0, 0, 1, 2]
    expect = ["1000000000", "1111110000", "1111111111", "0000000000"]
    host = match_predictions(np.array(pcls, np.float32), np.array(lcls, np.float32), box_iou(np.array(labels, np.float32), np.array(preds, np.float32)), IOUV)
    assert rows_of(host) == expect
    tp, bi, bl = run(device, pred_rows(preds, pcls, 5), [4], labels, np.array(lcls, np.float32), np.zeros(3, np.float32), clip=(1000, 1000))
    assert rows_of(tp[0, :4]) == expect and rows_of(tp[0, 4:]) == ["0000000000"]
    assert bi[0].tolist() == [0.5, 0.75, 1.0, 0.0, 0.0] and bl[0].tolist() == [0, 1, 2, 0, -1]  # (all-zero column: the image's first label)
    # contention: the higher-ranked detection keeps a label although a later one overlaps it more, and a detection whose best label
    # is taken gets no second choice
    labels, lcls = [(0, 0, 100, 100), (10, 0, 110, 100)], [0, 0]
    preds, pcls = [(0, 0, 100, 62), (0, 0, 100, 95), (6, 0, 106, 100)], [0, 0, 0]
    expect = ["1110000000", "0001111111", "1111111110"]
    host = match_predictions(np.array(pcls, np.float32), np.array(lcls, np.float32), box_iou(np.array(labels, np.float32), np.array(preds, np.float32)), IOUV)
    assert rows_of(host) == expect
    tp, _, bl = run(device, pred_rows(preds, pcls, 3), [3], labels, np.array(lcls, np.float32), np.zeros(2, np.int64), clip=(1000, 1000))
    assert rows_of(tp[0]) == expect and bl[0].tolist() == [0, 0, 1]
    # an exact tie for first place goes to the label that comes first in tbox (two identical labels; the second image's come first)
    tp, bi, bl = run(device, np.concatenate((pred_rows([(0, 0, 50, 50)], [1], 2), pred_rows([(0, 0, 50, 50), (0, 0, 50, 50)], [1, 1], 2))), [1, 2],
                     [(0, 0, 50, 50)] * 4, np.ones(4, np.float32), np.array([1, 0, 1, 0]), clip=(64, 64))
    assert bl.tolist() == [[1, -1], [0, 0]] and rows_of(tp[:, :, 0]) == ["10", "10"] and bi.tolist() == [[1.0, 0.0], [1.0, 1.0]]


@pytest.mark.gpu
def test_single_cls_no_labels_and_one_threshold(device):
    labels = [(10, 10, 60, 60), (100, 100, 180, 160), (200, 20, 260, 90)]
    preds, pcls = [(11, 10, 60, 61), (100, 104, 180, 160), (150, 150, 170, 170)], [1, 2, 3]  # classes that all differ from the labels' 0
    r = pred_rows(preds, pcls, 4)
    tp, _, bl = run(device, r, [3], labels, np.zeros(3, np.float32), np.zeros(3, np.float32))
    assert not tp.any() and bl[0].tolist() == [0, 0, 0, -1]
    tp, bi, bl = run(device, r, [3], labels, np.zeros(3, np.float32), np.zeros(3, np.float32), single_cls=True)
    host = match_predictions(np.zeros(3, np.float32), np.zeros(3, np.float32), box_iou(np.array(labels, np.float32), np.array(preds, np.float32)), IOUV)
    assert host[:2, 0].all() and not host[2].any()
    assert np.array_equal(tp[0, :3].astype(bool), host) and not tp[0, 3].any() and bl[0].tolist() == [0, 1, 1, -1]
    # no labels at all: null label pointers
    tp, bi, bl = run(device, r, [3], np.zeros((0, 4), np.float32), np.zeros(0, np.float32), np.zeros(0, np.float32))
    assert tp.shape == (1, 4, 10) and not tp.any() and not bi.any() and (bl == -1).all()
    # one threshold
    tp, _, _ = run(device, r, [3], labels, np.zeros(3, np.float32), np.zeros(3, np.float32), iouv=[0.95], single_cls=True)
    iou = box_iou(np.array(labels, np.float32), np.array(preds, np.float32)).max(0)  # 0.961, 0.933, 0.04
    assert (iou >= np.float32(0.95)).tolist() == [True, False, False]
    assert tp.shape == (1, 4, 1) and tp[0, :, 0].tolist() == [1, 0, 0, 0]


@pytest.mark.gpu
def test_captured_launch_replays_on_new_rows(device):
    c = batch_case()
    lab = [torch.as_tensor(c[k]).to(device) for k in ("tbox", "tcls", "timg")]
    variants = [c["rows"]]
    for s in (1, 2):
        v = c["rows"].copy()
        v[:, :, :4] += np.random.default_rng(s).normal(0, 2, v[:, :, :4].shape).astype(np.float32)
        variants.append(v)
    bufs = nms_buffers(variants[0], c["counts"], device)
    eager = []
    for v in variants:
        bufs.out.copy_(torch.as_tensor(v))
        eager.append([t.clone() for t in H.val_match(bufs, *lab, IOUV, (CLIP_W, CLIP_H), want_best=True)])
    assert not torch.equal(eager[0][0], eager[1][0]) and not torch.equal(eager[1][1], eager[2][1])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = H.val_match(bufs, *lab, IOUV, (CLIP_W, CLIP_H), want_best=True)
    for v, e in zip(variants[1:], eager[1:]):
        bufs.out.copy_(torch.as_tensor(v))
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(outs, e))


# ---- c. the validator ---------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def val_setup(device):
    """Drone-YOLO-n on 7 images of 128 x 128: labels = the model's own fp32 detections at conf 0.25 for six of them, none for the last."""
    import drone_yolo_amd as D
    from drone_yolo_amd.utils.parity import seeded_state_dict

    model = D.DetectionModel("yolov8n-p2-repvgg.yaml", nc=10, verbose=False)
    model.load_state_dict(seeded_state_dict(model.state_dict(), 5, cls_bias=-1.2))
    model = model.to(device).eval()
    n, s = 7, 128
    img = torch.randint(0, 256, (n, 3, s, s), generator=torch.Generator().manual_seed(3), dtype=torch.uint8)
    pred = D.engine.predictor.DetectionPredictor(model, dict(conf=0.25, iou=0.7, max_det=40, dtype="fp32", device=0))
    res = pred(img.float() / 255.0)
    bi, cls, bb = [], [], []
    for i, r in enumerate(res[: n - 1]):
        b = r.boxes.data.cpu()
        bi.append(torch.full((len(b),), float(i))), cls.append(b[:, 5:6])
        xyxy = b[:, :4]
        bb.append(torch.stack(((xyxy[:, 0] + xyxy[:, 2]) / 2 / s, (xyxy[:, 1] + xyxy[:, 3]) / 2 / s, (xyxy[:, 2] - xyxy[:, 0]) / s, (xyxy[:, 3] - xyxy[:, 1]) / s), 1))
    data = dict(img=img, batch_idx=torch.cat(bi), cls=torch.cat(cls), bboxes=torch.cat(bb))
    assert len(data["cls"]) >= 10
    return model, data


def count_calls(monkeypatch):
    """Counting wrappers around the two matchers, wherever the validator looks them up."""
    import drone_yolo_amd.engine.validator as V
    import drone_yolo_amd.utils.metrics as M

    calls = dict(device=0, host=0)
    dev = getattr(H, "val_match", None)

    def val_match(*a, **k):
        calls["device"] += 1
        return dev(*a, **k)

    def host_match(*a, **k):
        calls["host"] += 1
        return match_predictions(*a, **k)

    monkeypatch.setattr(H, "val_match", val_match, raising=False)
    monkeypatch.setattr(M, "match_predictions", host_match)
    monkeypatch.setattr(V, "match_predictions", host_match)
    return calls


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,single_cls", [(torch.float32, False), (torch.float16, False), (torch.float32, True)], ids=["fp32", "fp16", "single_cls"])
def test_validator_device_match_equals_host_match(device, val_setup, monkeypatch, dtype, single_cls):
    from drone_yolo_amd.engine.trainer import TensorLoader
    from drone_yolo_amd.engine.validator import DetectionValidator

    model, data = val_setup
    if single_cls:
        data = dict(data, cls=torch.zeros_like(data["cls"]))  # (what single_cls makes of a dataset: every label is class 0)
    calls = count_calls(monkeypatch)
    args = dict(iou=0.7, max_det=300, single_cls=single_cls)
    host = DetectionValidator(dict(args, device_match=False))(model, TensorLoader(data, 4, 0, 1, shuffle=False), torch.device(device), dtype)
    assert calls["device"] == 0 and calls["host"] >= 6
    calls["host"] = 0
    dev = DetectionValidator(dict(args, device_match=True))(model, TensorLoader(data, 4, 0, 1, shuffle=False), torch.device(device), dtype)
    assert (calls["device"], calls["host"]) == (2, 0), calls  # once per batch of the 7 images at batch 4; never the host matcher
    assert dev == host, (dev, host)
    assert host["metrics/mAP50(B)"] > 0.1, host  # (the comparison is of real matches)


@pytest.mark.gpu
def test_model_val_passes_device_match_through(device, val_setup, monkeypatch):
    import drone_yolo_amd as D

    model, data = val_setup
    yolo = D.YOLO("yolov8n-p2-repvgg.yaml")
    yolo.model = model
    host = yolo.val(data=data, batch=4, dtype="fp32", iou=0.7, device=0)
    calls = count_calls(monkeypatch)
    dev = yolo.val(data=data, batch=4, dtype="fp32", iou=0.7, device=0, device_match=True)
    assert (calls["device"], calls["host"]) == (2, 0), calls
    assert dev == host and yolo.metrics is dev
