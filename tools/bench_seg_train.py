"""Times the training step of a segmentation model next to the detection step of the same scale, and the mask term's launch sequence
(dy_seg_loss) next to dy_detection_loss on the same label table (GPU box).
usage: python tools/bench_seg_train.py [--scale s] [--batch 64] [--imgsz 640] [--dtype bf16] [--steps 20] [--warmup 5] [--runs 30] [--mode both|step|loss]
       rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/bench_seg_train.py --mode loss --runs 10      # kernel times

One process.  ``step``: the P2 ``-seg`` model and its detection twin (seeded weights, nc 10) under ``DetectionTrainer.step`` on batches of
``synthetic-seg`` / ``synthetic`` (the same draws; the detection set lacks the index maps) -- the graphed step from the third call on; each
timed step is a host clock from the call to a device synchronise behind it, the two models ALTERNATE step by step after ``--warmup`` steps
each; medians and ranges.  ``loss``: the head maps, coefficient maps and prototypes of one training forward of the ``-seg`` model (as the
loss gets them: fp32 maps, prototypes in the storage type) and the label table and index maps of one batch; ``H.seg_loss(..., want_grad=True)``
behind a fixed owner map and ``H.detection_loss(..., want_owner=True, want_grad=True)`` alternate, device events around each call, median
and range of ``--runs``; then one profiled call of each (torch.profiler) gives the per-kernel line of the two sequences, and the cast of the
fp32 prototype gradient to the storage type (``H.grad_cast_scaled``) is timed the same way.  Prints one JSON line."""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--scale", default="s")
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--imgsz", type=int, default=640)
ap.add_argument("--dtype", default="bf16")
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--runs", type=int, default=30)
ap.add_argument("--mode", default="both", choices=["both", "step", "loss"])
ap.add_argument("--seed", type=int, default=0)
a = ap.parse_args()

import torch
from drone_yolo_amd import hip_ops as H
from drone_yolo_amd.engine.trainer import DetectionTrainer, load_dataset
from drone_yolo_amd.nn.tasks import DetectionModel, SegmentationModel
from drone_yolo_amd.utils.parity import seeded_state_dict

assert torch.cuda.is_available(), "bench_seg_train.py measures on an MI355X"
dev = torch.device("cuda", 0)
nc, B, S = 10, a.batch, a.imgsz


def stats(ms):
    return dict(median=round(statistics.median(ms), 3), min=round(min(ms), 3), max=round(max(ms), 3), n=len(ms))


def build(cls, yaml):
    m = cls(yaml, nc=nc, verbose=False)
    m.load_state_dict(seeded_state_dict(m.state_dict(), 7 + a.seed, cls_bias=-1.6))
    return m


def batches(data, n):
    out = []
    for it in range(n):
        sel = torch.arange(it * B, (it + 1) * B) % data["img"].shape[0]
        rows = torch.isin(data["batch_idx"].long(), sel)
        remap = torch.full((data["img"].shape[0],), -1, dtype=torch.long)
        remap[sel] = torch.arange(B)
        out.append(dict(img=data["img"][sel].to(dev), batch_idx=remap[data["batch_idx"][rows].long()].float(), cls=data["cls"][rows], bboxes=data["bboxes"][rows]))
        order = torch.argsort(out[-1]["batch_idx"], stable=True)  # an image's labels contiguous and in dataset order, as TensorLoader yields them
        for k in ("batch_idx", "cls", "bboxes"):
            out[-1][k] = out[-1][k][order]
        if "masks" in data:
            out[-1]["masks"] = data["masks"][sel]
    return out


out = dict(scale=a.scale, batch=B, imgsz=S, dtype=a.dtype)
n_img = B * 2
seg_data, det_data = load_dataset(f"synthetic-seg:{n_img}", S, nc, a.seed), load_dataset(f"synthetic:{n_img}", S, nc, a.seed)
seg_model = build(SegmentationModel, f"yolov8{a.scale}-p2-repvgg-seg.yaml")

if a.mode in ("both", "step"):
    det_model = build(DetectionModel, f"yolov8{a.scale}-p2-repvgg.yaml")
    args = dict(optimizer="SGD", lr0=0.01, momentum=0.937, batch=B, nbs=B, dtype=a.dtype, warmup_epochs=0.0)
    runs = {"segment": (DetectionTrainer(seg_model, dict(args)), batches(seg_data, 2)), "detect": (DetectionTrainer(det_model, dict(args)), batches(det_data, 2))}
    ms = {k: [] for k in runs}
    for it in range(a.warmup + a.steps):
        for k, (tr, bs) in runs.items():  # alternating: both see the same minutes of the machine
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.step(dict(bs[it % 2]))
            torch.cuda.synchronize()
            if it >= a.warmup:
                ms[k].append((time.perf_counter() - t0) * 1e3)
    out["step_ms"] = {k: stats(v) for k, v in ms.items()}
    out["step_form"] = {k: tr.step_form() for k, (tr, _) in runs.items()}
    out["images_per_s"] = {k: round(B / statistics.median(v) * 1e3, 1) for k, v in ms.items()}
    seg_model = runs["segment"][0].model
    del runs, det_model

if a.mode in ("both", "loss"):
    seg_model = seg_model.to(dev).train()
    seg_model.train_dtype = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[a.dtype]
    batch = batches(seg_data, 1)[0]
    with torch.no_grad():
        feats, coefs, proto = seg_model.forward_train(batch["img"])
    feats, coefs, proto = [f.detach() for f in feats], [t.detach() for t in coefs], proto.detach()
    crit = seg_model.init_criterion()
    gt = crit.targets_to_gt(batch, B, (S, S)).to(dev)
    masks = batch["masks"].to(dev)
    strides = [float(s) for s in seg_model.stride]
    _, owner = H.detection_loss(feats, gt, strides, nc, want_owner=True)
    bufs = {}
    calls = {"seg_loss": lambda: H.seg_loss(owner, gt, coefs, proto, masks, (S, S), want_grad=True, buffers=bufs),
             "detection_loss": lambda: H.detection_loss(feats, gt, strides, nc, want_owner=True, want_grad=True)}
    gproto = calls["seg_loss"]()[2]
    one = torch.ones(1, device=dev)
    calls["proto_grad_cast"] = lambda: (H.grad_cast_scaled(gproto, proto.dtype, scale=one),)
    for f in calls.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(a.runs):
        for k, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    out["loss_ms"] = {k: stats(v) for k, v in ms.items()}
    out["labels"] = dict(rows=int((gt[..., 1:].sum(-1) > 0).sum()), gmax=int(gt.shape[1]), anchors=int(sum(f.shape[2] * f.shape[3] for f in feats)),
                         foreground=int((owner >= 0).sum()), proto=list(proto.shape), grad_proto_mb=round(gproto.numel() * 4 / 2**20, 1))
    out["loss_items"] = {k: [round(float(x), 4) for x in calls[k]()[0].cpu()] for k in ("seg_loss", "detection_loss")}
    try:  # the per-kernel line (device time of one call, by kernel name)
        from torch.profiler import ProfilerActivity, profile

        lines = {}
        for k, f in calls.items():
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                f()
                torch.cuda.synchronize()
            lines[k] = {e.key.split("(")[0].replace("dy::", "").replace("void ", ""): round(e.device_time_total, 1) for e in prof.key_averages() if e.device_time_total > 0}
        out["kernel_us"] = lines
    except Exception as exc:  # (a build of torch without the device tracer: the rocprofv3 line of the usage text gives the same table)
        out["kernel_us"] = f"not measured in-process ({type(exc).__name__}: {exc})"

print(json.dumps(out))
