"""Times YOLO.val of a pose model with the matching on the device (dy_val_match + dy_val_oks_match) and on the host, and the kernels of the
validator's post-processing on their own (GPU box).
usage: python tools/bench_poseval.py [--images 16] [--imgsz 640] [--batch 8] [--scale s] [--dtype f16x2] [--labels 12] [--runs 5] [--rounds 2]
       python tools/bench_poseval.py --mode kernels

The P2 pose model with seeded weights; the images live on the device, the labels are built from the model's own detections (the `--labels`
highest-scored rows of the single-label NMS: their boxes and their keypoints, all visible), so that matches exist.  `--mode both` (default)
starts one fresh child process per mode and round, alternating device / host; a child runs one warm-up validation (weight packing, workspaces)
and then `--runs` timed ones, each from the call of YOLO.val to its returned dict (which ends in a device-to-host copy, so nothing is left in
flight).  The parent commit cannot validate a pose model: the host restatement of the reference's data flow (device_match=False) is the
comparison.  `--mode kernels`: per batch, the device time (events, median of `--runs` after a warm-up) of the validator's NMS call
(ops.non_max_suppression with multi_label at conf 0.001), of hip_ops.val_match and of hip_ops.val_oks_match (the dense-plus-index form, with the
label conversions of the wrapper), next to the candidate counts per image.  Prints one JSON line."""
import argparse, json, os, subprocess, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--images", type=int, default=16)
ap.add_argument("--imgsz", type=int, default=640)
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--scale", default="s")
ap.add_argument("--dtype", default="f16x2", help="storage type of the model pass (cfg/default.yaml: dtype)")
ap.add_argument("--labels", type=int, default=12, help="labels per image (the model's highest-scored detections)")
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--mode", default="both", choices=["both", "device", "host", "kernels"])
ap.add_argument("--seed", type=int, default=0)
a = ap.parse_args()

if a.mode == "both":  # the parent never opens the device: one fresh child per (round, mode)
    res = {"device": [], "host": []}
    dicts = {}
    for _ in range(a.rounds):
        for m in ("device", "host"):
            cmd = [sys.executable, os.path.abspath(__file__), "--mode", m] + [f"--{k}={getattr(a, k)}" for k in ("images", "imgsz", "batch", "scale", "dtype", "labels", "runs", "seed")]
            line = subprocess.run(cmd, check=True, capture_output=True, text=True).stdout.strip().splitlines()[-1]
            r = json.loads(line)
            res[m] += r["ms"]
            dicts[m] = r["metrics"]
            info = {k: r[k] for k in ("labels_total", "rows_kept")}
    print(json.dumps(dict(images=a.images, imgsz=a.imgsz, batch=a.batch, scale=a.scale, dtype=a.dtype, runs=a.runs, rounds=a.rounds, **info,
                          device_ms=res["device"], host_ms=res["host"], device_range=[min(res["device"]), max(res["device"])],
                          host_range=[min(res["host"]), max(res["host"])], disjoint=max(res["device"]) < min(res["host"]) or max(res["host"]) < min(res["device"]),
                          dicts_equal=dicts["device"] == dicts["host"], metrics=dicts["device"])))
    sys.exit(0)

import numpy as np
import torch
import drone_yolo_amd as D
from drone_yolo_amd import hip_ops as H
from drone_yolo_amd.engine.predictor import resolve_dtype
from drone_yolo_amd.engine.validator import PoseValidator, pose_label_kpts
from drone_yolo_amd.nn.tasks import PoseModel
from drone_yolo_amd.utils import ops
from drone_yolo_amd.utils.metrics import OKS_SIGMA
from drone_yolo_amd.utils.parity import seeded_state_dict

dev = torch.device("cuda", 0)
dtype = resolve_dtype(a.dtype)
nc, s = 1, a.imgsz
yolo = D.YOLO(f"yolov8{a.scale}-p2-repvgg-pose.yaml")
yolo.model = PoseModel(f"yolov8{a.scale}-p2-repvgg-pose.yaml", nc=nc, verbose=False)
yolo.model.load_state_dict(seeded_state_dict(yolo.model.state_dict(), 5, cls_bias=-1.2))
assert yolo.model.yaml["nc"] == nc
kpt_shape = tuple(yolo.model.kpt_shape)
nkpt, ndim = kpt_shape
sigma = OKS_SIGMA if list(kpt_shape) == [17, 3] else np.ones(nkpt) / nkpt
model = yolo.model.to(dev).eval()
img = torch.randint(0, 256, (a.images, 3, s, s), generator=torch.Generator().manual_seed(a.seed), dtype=torch.uint8).to(dev)


def passes():
    """The fp32 (N, 4 + nc + nk, A) tensor of every batch through the validator's own model pass."""
    det = model.model[-1]
    fuse_tail = getattr(det, "fuse_tail", False)
    out = []
    for s0 in range(0, a.images, a.batch):
        with torch.no_grad():
            det.fuse_tail = False
            y, _ = model._predict_once((img[s0 : s0 + a.batch].float() / 255.0).contiguous(), image_dtype=dtype)
        out.append(y.float().contiguous())
    det.fuse_tail = fuse_tail
    return out


bi, cls, bb, kp = [], [], [], []
batches = passes()
for n0, y in enumerate(batches):
    bufs = ops.non_max_suppression(y, 0.01, 0.7, nc=nc, max_det=a.labels, return_padded=True)
    counts, rows, index = bufs.count.cpu().tolist(), bufs.out.cpu(), bufs.index.cpu().long()
    yk = y[:, 4 + nc :].cpu()
    for j, k in enumerate(counts):
        r = rows[j, :k]
        bi.append(torch.full((k,), float(n0 * a.batch + j))), cls.append(r[:, 5:6])
        bb.append(torch.stack(((r[:, 0] + r[:, 2]) / 2 / s, (r[:, 1] + r[:, 3]) / 2 / s, (r[:, 2] - r[:, 0]) / s, (r[:, 3] - r[:, 1]) / s), 1))
        k3 = yk[j][:, index[j, :k]].t().reshape(k, nkpt, ndim)
        kp.append(torch.cat((k3[..., :2] / s, torch.full((k, nkpt, 1), 2.0)), 2))
data = dict(img=img, batch_idx=torch.cat(bi), cls=torch.cat(cls), bboxes=torch.cat(bb), keypoints=torch.cat(kp))

if a.mode == "kernels":
    lim = torch.tensor((s, s, s, s), dtype=torch.float32, device=dev)
    iouv = np.linspace(0.5, 0.95, 10)
    v = PoseValidator()
    per_batch = []
    for n0, y in enumerate(batches):
        sel = (data["batch_idx"] >= n0 * a.batch) & (data["batch_idx"] < (n0 + 1) * a.batch)
        tbox = v._labels(data["bboxes"][sel].to(dev), s, s, lim)
        tkpt = pose_label_kpts(data["keypoints"][sel].to(dev), s, s, lim)
        tcls, timg = data["cls"][sel].view(-1).to(dev), (data["batch_idx"][sel] - n0 * a.batch).to(torch.int32).to(dev)

        def nms():
            return ops.non_max_suppression(y, 0.001, 0.7, nc=nc, multi_label=True, max_det=300, return_padded=True)

        bufs = nms()  # warm-up
        H.val_match(bufs, tbox, tcls, timg, iouv, (s, s))
        H.val_oks_match(bufs, y, kpt_shape, tbox, tkpt, tcls, timg, sigma, iouv, (s, s), nc=nc)
        torch.cuda.synchronize()
        cand = (y[:, 4 : 4 + nc] > 0.001).sum((1, 2)).cpu().tolist()
        t_nms, t_match, t_oks = [], [], []
        for _ in range(a.runs):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            e[0].record()
            bufs = nms()
            e[1].record()
            H.val_match(bufs, tbox, tcls, timg, iouv, (s, s))
            e[2].record()
            H.val_oks_match(bufs, y, kpt_shape, tbox, tkpt, tcls, timg, sigma, iouv, (s, s), nc=nc)
            e[3].record()
            torch.cuda.synchronize()
            t_nms.append(e[0].elapsed_time(e[1])), t_match.append(e[1].elapsed_time(e[2])), t_oks.append(e[2].elapsed_time(e[3]))

        def stat(t):
            return dict(median=round(float(np.median(t)), 4), range=[round(min(t), 4), round(max(t), 4)])

        per_batch.append(dict(candidates=cand, kept=bufs.count.cpu().tolist(), labels=int(sel.sum()), nms_ms=stat(t_nms), val_match_ms=stat(t_match), val_oks_match_ms=stat(t_oks)))
    print(json.dumps(dict(mode="kernels", images=a.images, imgsz=a.imgsz, batch=a.batch, scale=a.scale, dtype=a.dtype, anchors=int(batches[0].shape[2]), nc=nc,
                          kpt_shape=kpt_shape, runs=a.runs, batches=per_batch)))
    sys.exit(0)


def validate():
    kept = []

    def make(args):
        kept.append(PoseValidator(args))
        return kept[0]

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = yolo.val(validator=make, data=data, batch=a.batch, dtype=a.dtype, iou=0.7, max_det=300, device=0, device_match=(a.mode == "device"))
    return time.perf_counter() - t0, out, int(np.sum(kept[0].last_counts))


_, metrics, kept = validate()  # warm-up
ms = [round(validate()[0] * 1e3, 2) for _ in range(a.runs)]
print(json.dumps(dict(mode=a.mode, ms=ms, metrics=metrics, labels_total=int(len(data["cls"])), rows_kept=kept)))
