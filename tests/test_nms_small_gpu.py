"""dy_nms serves an image with one of two suppress kernels, chosen on the device by its candidate count: nms_small_kernel up to
``dy_nms_small_cap()`` candidates, nms_suppress_kernel above.  Every case here is compared with the oracle
(``oracle.drone_yolo_oracle.non_max_suppression(..., return_index=True)``) for EQUAL rows, kept anchor indices and counts, with zero
rows and index -1 past the count.  Candidate counts are built exactly (scores set so that exactly n anchors clear ``conf``) and
images on both sides of the cap share ONE batch, so both kernels serve images of the same call.

The inputs and the oracle's answers need no GPU: ``test_case_inputs_are_as_intended`` checks on the CPU that every case has the
candidate counts it is meant to have and that the early-stop cases really reach ``max_det``.
"""
import functools

import pytest
import torch

from drone_yolo_amd import _lib
from drone_yolo_amd import hip_ops as H
from oracle import drone_yolo_oracle as O

CONF = 0.25
NC = 4


def cap():
    return int(_lib.lib().dy_nms_small_cap())


def make_pred(counts, anchors, seed, nc=NC, ties=512, wh=(2.0, 80.0), second_label=0, clusters=0):
    """(len(counts), 4 + nc, anchors) predictions in which exactly counts[b] anchors of image b have a best class score above CONF.
    ``ties``: candidate scores are rounded to 1 / ties (exact ties for the stable-order rule); 0 = all scores of an image distinct.
    ``second_label``: that many of an image's candidates get a SECOND class above CONF (more candidates under multi_label only).
    ``clusters``: boxes are jittered copies of that many objects (what a detector emits: most candidates are suppressed)."""
    g = torch.Generator().manual_seed(seed)
    batch = len(counts)
    xy = torch.rand(batch, 2, anchors, generator=g) * 600 + 20
    box_wh = torch.rand(batch, 2, anchors, generator=g) * (wh[1] - wh[0]) + wh[0]
    if clusters:
        who = torch.randint(0, clusters, (batch, 1, anchors), generator=g).expand(batch, 2, anchors)
        xy = torch.gather(xy[:, :, :clusters], 2, who) + torch.rand(batch, 2, anchors, generator=g) * 8
        box_wh = torch.gather(box_wh[:, :, :clusters], 2, who) + 30 + torch.rand(batch, 2, anchors, generator=g) * 8
    sc = torch.rand(batch, nc, anchors, generator=g) * 0.2  # nobody clears CONF ...
    for b, n in enumerate(counts):
        who = torch.randperm(anchors, generator=g)[:n]  # ... but these n anchors, in one random class each
        cls = torch.randint(0, nc, (n,), generator=g)
        if ties:
            s = torch.round((0.3 + 0.7 * torch.rand(n, generator=g)) * ties) / ties
        else:
            s = 0.3 + 0.7 * (torch.randperm(n, generator=g).float() + 0.5) / max(n, 1)
        sc[b, cls, who] = s
        if second_label:
            m = min(second_label, n)
            sc[b, (cls[:m] + 1) % nc, who[:m]] = s[:m] - 0.03125  # still > CONF, below the first label: the best class stays
    return torch.cat((xy, box_wh, sc), 1).contiguous()


def mixed_counts():
    c = cap()
    return [0, 1, 63, 64, 65, c - 1, c, c + 1, 4 * c]


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (pred, kwargs of the NMS call, what the case is for).  Built once; the CPU test and the GPU tests share them."""
    c = cap()
    A = 8 * c
    out = {}
    out["mixed"] = (make_pred(mixed_counts(), A, 1), dict(max_det=300), "counts around 64 and around the cap in one batch")
    out["mixed_deep"] = (make_pred(mixed_counts(), A, 2), dict(max_det=1500), "the same with a kept list of up to 1500 boxes (the long kept-list loop of the scan)")
    out["ties"] = (make_pred([c - 3, 700, 2 * c], A, 3, ties=16), dict(max_det=300), "scores on a grid of 1/16: long runs of exact ties")
    out["clusters"] = (make_pred([c - 1, c, c + 1, 3 * c, 130], A, 10, clusters=24), dict(max_det=300), "jittered copies of 24 objects: most candidates are suppressed, every chunk is scanned")
    out["crowd"] =(make_pred([c - 100, c, 3 * c], A, 4, wh=(2.0, 10.0)), dict(max_det=300), "small boxes: more than max_det survive (early stop)")
    out["max_nms_below_cap"] = (make_pred([c - 24, c // 2, 3 * c], A, 5, ties=0), dict(max_det=300, max_nms=c // 2 - 12), "the max_nms cut below the cap, distinct scores")
    out["agnostic"] = (make_pred([c - 1, 200, c + 40], A, 6), dict(max_det=300, agnostic=True), "no class offset")
    out["class_mask"] = (make_pred([c, 3 * c, 90], A, 7), dict(max_det=300, classes=[0, 2]), "a class filter: the count that decides the kernel is the filtered one")
    out["multi_label_few"] = (make_pred([c // 2 - 10, 70, 0], A, 8, second_label=c // 4), dict(max_det=300, multi_label=True), "multi_label on the small path")
    out["multi_label_many"] = (make_pred([c - 200, 3 * c, c // 2], A, 9, second_label=c), dict(max_det=300, multi_label=True), "multi_label on both paths in one call")
    return out


def oracle(pred, kw):
    kw = dict(kw)
    return O.non_max_suppression(pred, CONF, 0.7, nc=NC, return_index=True, **kw)


def candidate_counts(pred, kw):
    """Candidates per image as dy_nms counts them: before the max_nms cut, after the class filter."""
    s = pred[:, 4:]
    if kw.get("multi_label"):
        ok = s > CONF
    else:
        best, j = s.max(1)
        ok = (best > CONF)[:, None, :] & (torch.arange(s.shape[1])[None, :, None] == j[:, None, :])
    if kw.get("classes") is not None:
        keep = torch.zeros(s.shape[1], dtype=torch.bool)
        keep[kw["classes"]] = True
        ok = ok & keep[None, :, None]
    return ok.sum((1, 2)).tolist()


def test_case_inputs_are_as_intended():
    c = cap()
    assert c >= 128 and c & (c - 1) == 0
    cs = cases()
    assert candidate_counts(cs["mixed"][0], {}) == [0, 1, 63, 64, 65, c - 1, c, c + 1, 4 * c]
    assert candidate_counts(cs["mixed_deep"][0], {}) == mixed_counts()
    for name, (pred, kw, _) in cs.items():
        n = candidate_counts(pred, kw)
        assert min(n) <= c < max(n) or name == "multi_label_few", f"{name}: one call must hold images of both kernels, has {n}"
    assert max(candidate_counts(*cs["multi_label_few"][:2])) <= c
    assert candidate_counts(*cs["multi_label_few"][:2])[0] == c // 2 - 10 + c // 4  # the second labels are candidates of their own
    assert candidate_counts(*cs["class_mask"][:2])[0] < c < candidate_counts(cs["class_mask"][0], {})[0] + 1
    # the early stop is really reached, on both sides of the cap; the deep case builds kept lists of more than 1000 boxes
    rows, _ = oracle(*cs["crowd"][:2])
    more, _ = oracle(cs["crowd"][0], dict(max_det=100000))
    assert [len(r) for r in rows] == [300, 300, 300] and all(len(m) > 300 for m in more)
    clu, _ = oracle(*cs["clusters"][:2])
    assert all(0 < len(r) < 300 and len(r) < n for r, n in zip(clu, candidate_counts(cs["clusters"][0], {}))), [len(r) for r in clu]
    assert all(4 * len(r) < n for r, n in zip(clu[:4], candidate_counts(cs["clusters"][0], {})))  # the large images lose most candidates
    deep, _ = oracle(*cs["mixed_deep"][:2])
    assert all(len(r) > 1000 for r in deep[5:])
    # the max_nms cut bites on the small path (an image at or below the cap with more candidates than max_nms)
    n = candidate_counts(*cs["max_nms_below_cap"][:2])
    assert cs["max_nms_below_cap"][1]["max_nms"] < n[1] <= c and n[0] <= c < n[2]
    # ties: most candidates share their score with another one
    s = cs["ties"][0][1, 4:].amax(0)
    s = s[s > CONF]
    assert len(s) == 700 and len(torch.unique(s)) <= 16


def run_device(pred, kw, device, bufs=None):
    kw = dict(kw)
    classes = kw.pop("classes", None)
    mask = None
    if classes is not None:
        mask = torch.zeros(NC, dtype=torch.uint8)
        mask[classes] = 1
        mask = mask.to(device)
    return H.nms(pred, CONF, 0.7, max_det=kw.get("max_det", 300), max_nms=kw.get("max_nms", 30000), agnostic=kw.get("agnostic", False),
                 classes_mask=mask, multi_label=kw.get("multi_label", False), bufs=bufs)


def check_against_oracle(name, pred, kw, bufs):
    exp, exp_idx = oracle(pred, kw)
    counts = bufs.count.cpu().tolist()
    out, index = bufs.out.cpu(), bufs.index.cpu()
    print(f"{name}: candidates {candidate_counts(pred, kw)} kept {counts}")
    assert counts == [len(e) for e in exp], f"{name}: counts {counts} vs {[len(e) for e in exp]}"
    for i, c in enumerate(counts):
        assert torch.equal(index[i, :c].long(), exp_idx[i]), f"{name}: image {i}: kept anchor indices differ"
        assert torch.equal(out[i, :c], exp[i]), f"{name}: image {i}: rows differ"
        assert float(out[i, c:].abs().sum()) == 0 and bool((index[i, c:] == -1).all()), f"{name}: image {i}: rows past the count"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mixed", "mixed_deep", "ties", "clusters", "crowd", "max_nms_below_cap", "agnostic", "class_mask", "multi_label_few", "multi_label_many"])
def test_nms_small_and_large_match_oracle(name, device):
    pred, kw, _ = cases()[name]
    bufs = run_device(pred.to(device), kw, device)
    torch.cuda.synchronize()
    check_against_oracle(name, pred, kw, bufs)


@pytest.mark.gpu
def test_nms_graph_replays_leave_identical_buffers(device):
    """The whole of dy_nms (counts reset, filter, both suppress kernels) is captured in a hipGraph; two consecutive replays leave the
    same buffers as each other and as the oracle, also after the buffers were overwritten in between."""
    pred, kw, _ = cases()["mixed"]
    x = pred.to(device)
    bufs = run_device(x, kw, device)  # eager first: the library's one-time kernel attributes are set outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        run_device(x, kw, device, bufs=bufs)
    snaps = []
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        snaps.append((bufs.out.clone(), bufs.count.clone(), bufs.index.clone()))
        check_against_oracle("mixed (replay)", pred, kw, bufs)
        bufs.out.fill_(7.0), bufs.count.fill_(-3), bufs.index.fill_(5)
    assert all(torch.equal(a, b) for a, b in zip(*snaps))
