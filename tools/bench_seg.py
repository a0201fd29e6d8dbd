"""Times the segmentation path (GPU box): mask assembly against the same result composed from torch ops, and a predict call with and without masks.
usage: python tools/bench_seg.py [--rounds 10] [--scale s] [--dtype float16] [--imgsz 640] [--batches 1,16] [--dets 30,300]

Drone-YOLO `-seg` at imgsz^2 (the prototypes come from the stride-4 map, so they are imgsz / 2 a side).  A and B alternate in one process after
warm-up and are timed with device events; each figure is the median over `--rounds` rounds, with the smallest and largest beside it.
  (a) masks   per (batch, detections per image, box size: 3-18 % or 30-90 % of the image a side): A = torch ops on the device, image by image as the reference does (matmul, crop multiply,
              F.interpolate bilinear, gt), B = one dy_process_mask launch; the two results are compared; GB/s of B against the bytes the
              algorithm must move: the 128-byte proto pixels under the boxes (once per detection) plus one byte per output pixel.
  (b) predict host clock around predict() on one batch, results built: the `-seg` model (masks) against its detection twin (no masks), and the
              device time of the recorded pass of each (the difference is Proto + the coefficient branches + the gather).
Prints one JSON line."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--scale", default="s")
ap.add_argument("--dtype", default="float16")
ap.add_argument("--imgsz", type=int, default=640)
ap.add_argument("--batches", default="1,16")
ap.add_argument("--dets", default="30,300")
ap.add_argument("--no-e2e", action="store_true")
a = ap.parse_args()
assert torch.cuda.is_available(), "tools/bench_seg.py needs an MI355X"
dev = torch.device("cuda", 0)

from drone_yolo_amd import YOLO
from drone_yolo_amd import hip_ops as H

S, MH, MAX_DET = a.imgsz, a.imgsz // 2, 300


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


def torch_masks(protos_chw, coef, boxes, shape):
    """ops.process_mask(upsample=True) of the reference, restated with the same torch ops on the device (utils/ops.py:660-709)."""
    c, mh, mw = protos_chw.shape
    m = (coef @ protos_chw.view(c, -1)).view(-1, mh, mw)
    b = boxes * torch.tensor([mw / shape[1], mh / shape[0], mw / shape[1], mh / shape[0]], device=boxes.device)
    x1, y1, x2, y2 = torch.chunk(b[:, :, None], 4, 1)
    r = torch.arange(mw, device=m.device, dtype=x1.dtype)[None, None, :]
    cc = torch.arange(mh, device=m.device, dtype=x1.dtype)[None, :, None]
    m = m * ((r >= x1) * (r < x2) * (cc >= y1) * (cc < y2))
    return F.interpolate(m[None], shape, mode="bilinear", align_corners=False)[0].gt_(0.0)


res = {"imgsz": S, "proto_hw": MH, "scale": a.scale, "dtype": a.dtype, "masks": [], "predict": {}}
gen = torch.Generator().manual_seed(0)
for n, k, (lo, hi) in [(n, k, sz) for n in [int(v) for v in a.batches.split(",")] for k in [int(v) for v in a.dets.split(",")] for sz in ((0.03, 0.18), (0.3, 0.9))]:
    if True:
        protos = torch.randn(n, MH, MH, 32, generator=gen).to(dev)
        coef = torch.randn(n, MAX_DET, 32, generator=gen)
        c = torch.rand(n, MAX_DET, 2, generator=gen) * S
        wh = torch.rand(n, MAX_DET, 2, generator=gen) * (hi - lo) * S + lo * S
        boxes = torch.cat([c - wh / 2, c + wh / 2], 2) + 0.137
        side = torch.cat([boxes, coef], 2).to(dev).contiguous()
        counts = [k] * n
        count = torch.tensor(counts, dtype=torch.int32, device=dev)
        pv, pchw = protos.permute(0, 3, 1, 2), protos.permute(0, 3, 1, 2).contiguous()
        keep = {}

        def run_a():
            keep["a"] = [torch_masks(pchw[i], side[i, :k, 4:], side[i, :k, :4], (S, S)) for i in range(n)]

        def run_b():
            keep["b"] = H.process_mask(pv, side, count, counts, (S, S), ratio=(MH / S, MH / S))

        t = ab({"torch_ops": run_a, "dy_process_mask": run_b}, a.rounds)
        ref = torch.cat(keep["a"]).to(torch.uint8)
        differ = int((ref != keep["b"]).sum())
        bx = boxes[:, :k].clamp(0, S) * (MH / S)
        under = float(((bx[..., 2] - bx[..., 0] + 1) * (bx[..., 3] - bx[..., 1] + 1)).sum()) * 128
        must = under + n * k * S * S
        row = {"batch": n, "dets_per_image": k, "box_side_share": [lo, hi], "torch_ops_ms": stat(t["torch_ops"]), "dy_process_mask_ms": stat(t["dy_process_mask"]),
               "differing_pixels": differ, "pixels": int(ref.numel()), "bytes_must_move": int(must),
               "dy_process_mask_GBps": round(must / (float(np.median(t["dy_process_mask"])) * 1e-3) / 1e9, 1)}
        res["masks"].append(row)
        del keep, protos, pchw, ref
        torch.cuda.empty_cache()

if not a.no_e2e:
    x = torch.rand(16, 3, S, S, generator=gen).to(dev)
    for name, yaml_name in (("seg", f"yolov8{a.scale}-p2-repvgg-seg.yaml"), ("detect", f"yolov8{a.scale}-p2-repvgg.yaml")):
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
                                "box_area_share": round(float(np.mean([float(((q.boxes.xyxy[:, 2] - q.boxes.xyxy[:, 0]) * (q.boxes.xyxy[:, 3] - q.boxes.xyxy[:, 1])).mean()) / (S * S) for q in r if len(q)])), 3)}
print(json.dumps(res))
