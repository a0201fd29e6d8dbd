"""Times the oriented-box post-processing (GPU box): the reference's chain as torch ops on the device against the three kernels, and a predict call
of an `-obb` model against its detection twin.
usage: python tools/bench_obb.py [--rounds 10] [--scale s] [--dtype float16] [--imgsz 640] [--batches 1,16] [--cands 30,300,3000]

Drone-YOLO P2 anchors at imgsz^2 (34,000 at 640), nc 10.  A and B alternate in one process after warm-up and are timed with device events; each
figure is the median over `--rounds` rounds, with the smallest and largest beside it.
  (a) chain   per (batch, candidates per image): A = what the reference runs, as torch ops on the device, image by image: dist2rbox on the
              full map (utils/tal.py), the candidate filter and the class offset (utils/ops.py:250-308), batch_probiou n x n, triu, the pick
              (ops.py:160-167), regularize_rboxes + scale_boxes(xywh=True); B = dy_obb_decode + dy_nms_rotated + dy_scale_rboxes (B first restores
              the two centre rows dy_obb_decode turns in place: one small copy inside its time).  Kept anchors and rows of the two are compared.
  (b) decode  dy_obb_decode alone per batch: the bytes it must move (per anchor one logit read, two centre floats read and written, one angle
              written: 24 B) over its time.
  (c) predict host clock around predict() on one batch of 16, results built: the `-obb` model against its detection twin, and the device time of
              the recorded pass of each (the difference is the angle branches, dy_obb_decode and the two rotated kernels in place of dy_nms / dy_scale_boxes).
Prints one JSON line."""
import argparse, json, math, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--scale", default="s")
ap.add_argument("--dtype", default="float16")
ap.add_argument("--imgsz", type=int, default=640)
ap.add_argument("--batches", default="1,16")
ap.add_argument("--cands", default="30,300,3000")
ap.add_argument("--decode-batches", default="1,16,256")
ap.add_argument("--no-e2e", action="store_true")
a = ap.parse_args()
assert torch.cuda.is_available(), "tools/bench_obb.py needs an MI355X"
dev = torch.device("cuda", 0)

from drone_yolo_amd import YOLO
from drone_yolo_amd import hip_ops as H

S, NC, MAX_DET, CONF, IOU, MAX_WH = a.imgsz, 10, 300, 0.25, 0.7, 7680.0
STRIDES = (4, 8, 16, 32)
HW = [(S // s, S // s) for s in STRIDES]
A = sum(h * w for h, w in HW)


def stat(ts):
    return {"median": round(float(np.median(ts)), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def ab(fns, rounds, warm=2):
    for _ in range(warm):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k].append(timed(fn))
    return out


def probiou(b1, b2, eps=1e-7):
    """batch_probiou (utils/metrics.py:244-275) with the same torch ops."""
    def cov(b):
        aa, bb, r = b[:, 2:3].pow(2) / 12, b[:, 3:4].pow(2) / 12, b[:, 4:5]
        cos, sin = r.cos(), r.sin()
        return aa * cos.pow(2) + bb * sin.pow(2), aa * sin.pow(2) + bb * cos.pow(2), (aa - bb) * cos * sin
    x1, y1 = b1[:, 0:1], b1[:, 1:2]
    x2, y2 = b2[:, 0][None], b2[:, 1][None]
    a1, bb1, c1 = cov(b1)
    a2, bb2, c2 = (t.squeeze(-1)[None] for t in cov(b2))
    det = (a1 + a2) * (bb1 + bb2) - (c1 + c2).pow(2)
    t1 = (((a1 + a2) * (y1 - y2).pow(2) + (bb1 + bb2) * (x1 - x2).pow(2)) / (det + eps)) * 0.25
    t2 = (((c1 + c2) * (x2 - x1) * (y1 - y2)) / (det + eps)) * 0.5
    t3 = (det / (4 * ((a1 * bb1 - c1.pow(2)).clamp_(0) * (a2 * bb2 - c2.pow(2)).clamp_(0)).sqrt() + eps) + eps).log() * 0.5
    bd = (t1 + t2 + t3).clamp(eps, 100.0)
    return 1 - (1.0 - (-bd).exp() + eps).sqrt()


def torch_chain(dist, logit, scores, anchors, strides, params):
    """The reference's post-processing of one batch with torch ops on the device; returns per image (rows (k, 7), kept anchors)."""
    angle = (logit.sigmoid() - 0.25) * math.pi  # (n, 1, A)
    lt, rb = dist.split(2, 1)
    cos, sin = angle.cos(), angle.sin()
    xf, yf = ((rb - lt) / 2).split(1, 1)
    xy = torch.cat([xf * cos - yf * sin, xf * sin + yf * cos], 1) + anchors
    box = torch.cat([xy, lt + rb], 1) * strides
    pred = torch.cat([box, scores, angle], 1).transpose(-1, -2)
    xc = scores.amax(1) > CONF
    out = []
    for i in range(pred.shape[0]):
        idx = xc[i].nonzero()[:, 0]
        x = pred[i][idx]
        conf, j = x[:, 4 : 4 + NC].max(1, keepdim=True)
        x = torch.cat((x[:, :4], conf, j.float(), x[:, -1:]), 1)
        c = x[:, 5:6] * MAX_WH
        boxes = torch.cat((x[:, :2] + c, x[:, 2:4], x[:, -1:]), -1)
        order = torch.argsort(x[:, 4], descending=True)
        ious = probiou(boxes[order], boxes[order]).triu_(diagonal=1)
        pick = order[torch.nonzero((ious >= IOU).sum(0) <= 0).squeeze_(-1)][:MAX_DET]
        x, t = x[pick], x[pick, 6]
        swap = t % math.pi >= math.pi / 2
        w_, h_ = torch.where(swap, x[:, 3], x[:, 2]), torch.where(swap, x[:, 2], x[:, 3])
        gain, px, py, cw, ch = params[i]
        rows = torch.stack([((x[:, 0] - px) / gain).clamp(0, cw), ((x[:, 1] - py) / gain).clamp(0, ch), (w_ / gain).clamp(0, cw), (h_ / gain).clamp(0, ch),
                            t % (math.pi / 2), x[:, 4], x[:, 5]], -1)
        out.append((rows, idx[pick]))
    return out


def make_inputs(n, k, gen):
    """dist / angle logits / class scores of n images with k candidates each: jittered copies of k / 6 objects, so most candidates are suppressed."""
    anchors = torch.cat([torch.stack(torch.meshgrid(torch.arange(w) + 0.5, torch.arange(h) + 0.5, indexing="xy"), -1).reshape(-1, 2) for h, w in HW]).t()[None]  # (1, 2, A)
    strides = torch.cat([torch.full((h * w,), float(s)) for (h, w), s in zip(HW, STRIDES)])[None, None]
    dist = torch.rand(n, 4, A, generator=gen) * 4 + 0.5
    logit = torch.randn(n, 1, A, generator=gen)
    scores = torch.rand(n, NC, A, generator=gen) * 0.2
    objs = max(k // 6, 1)
    for b in range(n):
        who = torch.randperm(A, generator=gen)[:k]
        o = torch.randint(0, objs, (k,), generator=gen)
        centre = torch.rand(objs, 2, generator=gen) * (S - 80) + 40
        size = torch.rand(objs, 2, generator=gen) * 40 + 12
        ang = torch.randn(objs, generator=gen)
        st, an = strides[0, 0, who], anchors[0, :, who]
        # distances that put the rotated box of anchor `who` on its object (dist2rbox inverted), plus jitter
        th = (torch.sigmoid(ang[o]) - 0.25) * math.pi
        d = (centre[o] + torch.rand(k, 2, generator=gen) * 4).t() / st - an
        xf, yf = d[0] * th.cos() + d[1] * th.sin(), -d[0] * th.sin() + d[1] * th.cos()
        wh = (size[o] + torch.rand(k, 2, generator=gen) * 3).t() / st
        dist[b, 0, who], dist[b, 2, who] = wh[0] / 2 - xf, wh[0] / 2 + xf
        dist[b, 1, who], dist[b, 3, who] = wh[1] / 2 - yf, wh[1] / 2 + yf
        logit[b, 0, who] = ang[o] + torch.randn(k, generator=gen) * 0.02
        scores[b, torch.randint(0, NC, (k,), generator=gen), who] = 0.3 + 0.7 * (torch.randperm(k, generator=gen).float() + 0.5) / k
    return dist, logit, scores, anchors, strides


def level_maps(logit, n):
    out, a0 = [], 0
    for h, w in HW:
        buf = H.alloc_nhwc(n, 8, h, w, torch.float32, dev)
        buf[:, 0] = logit[:, 0, a0 : a0 + h * w].reshape(n, h, w).to(dev)
        out.append(buf[:, :1])
        a0 += h * w
    return out


res = {"imgsz": S, "anchors": A, "nc": NC, "conf": CONF, "iou": IOU, "chain": [], "decode": [], "predict": {}}
gen = torch.Generator().manual_seed(0)
for n in [int(v) for v in a.batches.split(",")]:
    for k in [int(v) for v in a.cands.split(",")]:
        dist, logit, scores, anchors, strides = (t.to(dev) for t in make_inputs(n, k, gen))
        params = torch.tensor([[1.0, 0.0, 0.0, float(S), float(S)]] * n, device=dev)
        lt, rb = dist.split(2, 1)
        pred0 = torch.cat([((anchors - lt) + (anchors + rb)) / 2 * strides, (lt + rb) * strides, scores], 1).contiguous()  # what Detect's decode leaves
        pred, levels = pred0.clone(), level_maps(logit, n)
        theta = torch.empty(n, A, device=dev)
        bufs = H.RNmsBuffers(n, A, MAX_DET, dev)
        keep = {}

        def run_a():
            keep["a"] = torch_chain(dist, logit, scores, anchors, strides, params.tolist())

        def run_b():
            pred[:, :2].copy_(pred0[:, :2])
            H.obb_decode(levels, STRIDES, pred, NC, theta=theta)
            H.nms_rotated(pred, theta, CONF, IOU, max_det=MAX_DET, max_wh=MAX_WH, nc=NC, bufs=bufs)
            H.scale_rboxes_(bufs, params)

        t = ab({"torch_ops": run_a, "kernels": run_b}, a.rounds)
        counts = bufs.count.tolist()
        same = all(len(ra) == c and torch.equal(ia.int(), bufs.index[i, :c]) for i, ((ra, ia), c) in enumerate(zip(keep["a"], counts)))
        diff = max([float((ra - bufs.out[i, : len(ra)]).abs().max()) for i, (ra, _) in enumerate(keep["a"]) if len(ra) and len(ra) == counts[i]] or [0.0])
        res["chain"].append({"batch": n, "candidates_per_image": k, "kept_per_image": round(float(np.mean(counts)), 1), "torch_ops_ms": stat(t["torch_ops"]),
                             "kernels_ms": stat(t["kernels"]), "same_kept_anchors": bool(same), "max_row_difference": diff})
        del keep
for n in [int(v) for v in a.decode_batches.split(",")]:
    logit = torch.randn(n, 1, A, generator=gen)
    pred, levels, theta = torch.rand(n, 4 + NC, A, device=dev), level_maps(logit, n), torch.empty(n, A, device=dev)
    t = ab({"dy_obb_decode": lambda: H.obb_decode(levels, STRIDES, pred, NC, theta=theta)}, a.rounds)["dy_obb_decode"]
    must = n * A * 24
    res["decode"].append({"batch": n, "ms": stat(t), "bytes_must_move": must, "GBps": round(must / (float(np.median(t)) * 1e-3) / 1e9, 1)})

if not a.no_e2e:
    x = torch.rand(16, 3, S, S, generator=gen).to(dev)
    for name, yaml_name in (("obb", f"yolov8{a.scale}-p2-repvgg-obb.yaml"), ("detect", f"yolov8{a.scale}-p2-repvgg.yaml")):
        y = YOLO(yaml_name)
        for m in y.model.model[-1].cv3:  # stock bias leaves no candidates: lift the class bias so that a few dozen rows survive per image
            m[-1].bias.data += 10.0
        kw = dict(device=0, dtype=a.dtype, conf=0.25, iou=0.7)
        for _ in range(3):
            r = y.predict(x, **kw)
        torch.cuda.synchronize()
        host = []
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            r = y.predict(x, **kw)
            torch.cuda.synchronize()
            host.append((time.perf_counter() - t0) * 1e3)
        p = y.predictor
        dev_ms = [timed(lambda: p.forward_device(x)) for _ in range(a.rounds)]
        res["predict"][name] = {"batch": 16, "predict_ms": stat(host), "recorded_pass_ms": stat(dev_ms), "rows_per_image": round(float(np.mean([len(q) for q in r])), 1),
                                "launches": len(p._compiled[next(iter(p._compiled))].plan.ops)}
print(json.dumps(res))
