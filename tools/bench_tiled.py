"""Times tiled inference on 4K frames (GPU box): the parent's per-frame stages against the batched slicer and the one-launch merge.
usage: python tools/bench_tiled.py [--rounds 10] [--frames 24] [--scale s] [--dtype float16] [--tile 1280] [--overlap 0.2] [--obb | --seg]

A synthetic 3840 x 2160 uint8 video, tile 1280, overlap 0.2 (eight tiles per frame).  Every comparison alternates A and B in one process
after warm-up and is timed with device events; each figure is the median over `--rounds` rounds, with the smallest and largest beside it.
  (a) merge   the merge stage alone on the same per-tile rows (objects seen by every tile that holds them, about 30 and about 300 rows per
              tile): A = dy_rows_to_pred + dy_nms (the parent chain, one frame), B = dy_tile_merge (one frame); B8 = dy_tile_merge on eight
              frames in one launch, per frame; U / W = dy_tile_fuse in mode union / wbf (one frame), U8 / W8 on eight frames, per frame.
  (b) slicer  eight frames: A = eight dy_tiles_u8_to_nchw_f32 launches, B = one dy_tiles_batch_u8_to_nchw_f32 launch; ms and GB/s written.
  (c) frames/s end to end over `--frames` frames (host clock around the whole loop, results materialised): A = TiledPredictor called frame by
              frame, B = predict(frames, tile=1280, batch=F, stream=True) for F = 1, 2, 4.
--obb: oriented boxes.  (a) gains R = dy_tile_merge_rotated (one frame) and R8 (eight frames, per frame) on the same objects as xywh rows with
an angle each -- the same counts, so the difference to B / B8 is the price of the ProbIoU predicate; (c) runs the `-obb` model of the scale
through predict(frames, tile=..., batch=F, stream=True) only (TiledPredictor is the detection task's).
--seg: segmentation, this row alone.  The frame masks of one frame on synthetic prototypes (K, 320, 320, 32) and about 30 rows per
tile: dy_tile_mask_owner + dy_tile_process_mask at stride 4 and 1, merge_mode suppress and union; beside them dy_process_mask to (tile, tile) for
the same kept rows, tile by tile -- what the package could do with them before.  Then frames/s of predict(frames, tile=..., batch=F, stream=True)
of the `-seg` model of the scale (yolov8<scale>-seg.yaml) at tile_mask_stride 4, F = 1, 2, 4.
Prints one JSON line."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--frames", type=int, default=24)
ap.add_argument("--scale", default="s")
ap.add_argument("--dtype", default="float16")
ap.add_argument("--tile", type=int, default=1280)
ap.add_argument("--overlap", type=float, default=0.2)
ap.add_argument("--no-e2e", action="store_true")
ap.add_argument("--obb", action="store_true")
ap.add_argument("--seg", action="store_true")
a = ap.parse_args()
assert torch.cuda.is_available(), "tools/bench_tiled.py needs an MI355X"
dev = torch.device("cuda", 0)

import drone_yolo_amd as D
from drone_yolo_amd import hip_ops as H
from drone_yolo_amd._lib import lib
from drone_yolo_amd.engine.tiling import TiledPredictor, tile_offsets

HF, WF, MAX_DET, KEEP, NC, THR = 2160, 3840, 300, 1000, 10, 0.7
offs = tile_offsets(HF, WF, a.tile, a.overlap)
K = len(offs)
offs_d = torch.tensor(offs, dtype=torch.int32, device=dev)
st = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731


def stat(ts):
    return {"median": round(float(np.median(ts)), 4), "min": round(min(ts), 4), "max": round(max(ts), 4)}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def ab(fns, rounds, warm=3):
    """Alternating runs of every function of ``fns`` per round; {name: [ms, ...]}."""
    for _ in range(warm):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ts[k].append(timed(fn))
    return ts


def scene_rows(seed, per_tile, frames):
    """Per-tile rows of `frames` frames: objects of 8-40 px scattered over the frame, each seen (with 2 % jitter) by every tile that holds it whole,
    about `per_tile` rows in a tile, in descending score."""
    rng = np.random.default_rng(seed)
    rows, counts = np.zeros((frames * K, MAX_DET, 6), np.float32), np.zeros((frames * K,), np.int32)
    n_obj = int(per_tile * HF * WF / (a.tile * a.tile))
    for f in range(frames):
        wh = rng.uniform(8, 40, (n_obj, 2))
        xy = np.stack([rng.uniform(0, WF - 40, n_obj), rng.uniform(0, HF - 40, n_obj)], 1)
        box = np.concatenate([xy, xy + wh], 1)
        sc, cls = rng.uniform(0.1, 0.99, n_obj), rng.integers(0, NC, n_obj)
        for k, (oy, ox) in enumerate(offs):
            inside = (box[:, 0] >= ox) & (box[:, 1] >= oy) & (box[:, 2] <= ox + a.tile) & (box[:, 3] <= oy + a.tile)
            i = np.nonzero(inside)[0]
            v = box[i] + rng.uniform(-0.02, 0.02, (len(i), 4)) * np.tile(wh[i], 2) - np.array([ox, oy, ox, oy])
            r = np.concatenate([np.clip(v, 0, a.tile), (sc[i] + rng.uniform(-0.01, 0.01, len(i)))[:, None], cls[i, None]], 1).astype(np.float32)
            r = r[np.argsort(-r[:, 4], kind="stable")][:MAX_DET]
            rows[f * K + k, : len(r)], counts[f * K + k] = r, len(r)
    return rows, counts


out = {"frame": [HF, WF], "tile": a.tile, "overlap": a.overlap, "tiles": K, "rounds": a.rounds, "merge": [], "slicer": None, "end_to_end": None}

# ---- --seg: the frame masks of a tiled segmentation model, and frames per second end to end --------------------------------------------------
if a.seg:
    mh = a.tile // 4
    rows, counts = scene_rows(30, 30, 1)
    rows_d, counts_d = torch.from_numpy(rows).to(dev), torch.from_numpy(counts).to(dev)
    g = torch.Generator(device="cpu").manual_seed(3)
    protos = torch.randn(K, mh, mh, 32, generator=g).to(dev).permute(0, 3, 1, 2)  # the NHWC view
    side = torch.cat([rows_d[:, :, :4], torch.randn(K, MAX_DET, 32, generator=g).to(dev)], 2).contiguous()
    seg = {"rows_per_tile": round(float(counts.mean()), 1), "masks": {}}
    fns = {}
    for mode in ("suppress", "union"):
        merged = H.tile_merge((rows_d, counts_d), offs_d, K, (HF, WF), NC, THR, 0, False, KEEP, mode=mode)
        index, count = merged.index.clone(), merged.count.clone()
        n = int(count[0])
        dest = torch.full((1, KEEP), -1, dtype=torch.int32, device=dev)
        dest[0, :n] = torch.arange(n, dtype=torch.int32, device=dev)
        seg["kept"] = n
        for s_ in (4, 1):
            buf = torch.empty((n, -(-HF // s_), -(-WF // s_)), dtype=torch.uint8, device=dev)

            def run(mode=mode, index=index, count=count, dest=dest, s_=s_, buf=buf, n=n):
                owner = H.tile_mask_owner((rows_d, counts_d), offs_d, K, (index, count), THR, 0, False, stitch=mode != "suppress")
                H.tile_process_mask(protos, side, counts_d, offs_d, owner, dest, n, (a.tile, a.tile), (HF, WF), s_, out=buf)

            fns[f"{mode}_stride{s_}"] = run
    # the same kept rows through dy_process_mask, tile by tile, to (tile, tile)
    merged = H.tile_merge((rows_d, counts_d), offs_d, K, (HF, WF), NC, THR, 0, False, KEEP)
    kept = merged.index[0, : int(merged.count[0])].long().cpu().numpy()
    side_k, counts_k = torch.zeros_like(side), np.zeros((K,), np.int32)
    for slot in np.sort(kept):
        k, r = divmod(int(slot), MAX_DET)
        side_k[k, counts_k[k]] = side[k, r]
        counts_k[k] += 1
    counts_kd = torch.from_numpy(counts_k).to(dev)
    pm_out = torch.empty((int(counts_k.sum()), a.tile, a.tile), dtype=torch.uint8, device=dev)
    fns["process_mask_per_tile"] = lambda: H.process_mask(protos, side_k, counts_kd, counts_k.tolist(), (a.tile, a.tile), ratio=(0.25, 0.25), out=pm_out)
    ts = ab(fns, a.rounds)
    seg["masks"] = {k: stat(v) for k, v in ts.items()}
    print(json.dumps(seg), file=sys.stderr, flush=True)
    del pm_out, fns
    if not a.no_e2e:
        from drone_yolo_amd.utils.parity import seeded_state_dict

        yolo = D.YOLO(f"yolov8{a.scale}-seg.yaml")
        yolo.model.load_state_dict(seeded_state_dict(yolo.model.state_dict(), 5, cls_bias=-1.2))
        video = [np.ascontiguousarray(f) for f in np.random.default_rng(2).integers(0, 256, (a.frames, HF, WF, 3), dtype=np.uint8)]

        def batched(F):
            return [len(r) for r in yolo.predict(video, tile=a.tile, tile_overlap=a.overlap, merge_iou=THR, merge_max_det=KEEP, batch=F, stream=True,
                                                 tile_mask_stride=4, conf=0.25, iou=0.7, dtype=a.dtype, device=0)]

        fps, boxes = {F: [] for F in (1, 2, 4)}, {}
        for F in fps:
            boxes[F] = int(sum(batched(F)))
        rounds = max(3, a.rounds // 2)
        for _ in range(rounds):
            for F in fps:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                batched(F)
                torch.cuda.synchronize()
                fps[F].append(a.frames / (time.perf_counter() - t0))
        seg["end_to_end"] = {"frames": a.frames, "scale": a.scale, "dtype": a.dtype, "rounds": rounds, "boxes": boxes,
                             "frames_per_s": {f"predict_batch{F}": stat(v) for F, v in fps.items()}}
    print(json.dumps({"frame": [HF, WF], "tile": a.tile, "overlap": a.overlap, "tiles": K, "rounds": a.rounds, "seg": seg}))
    sys.exit(0)

# ---- (a) the merge stage alone --------------------------------------------------------------------------------------------------------------
for per_tile in (30, 300):
    rows, counts = scene_rows(per_tile, per_tile, 8)
    rows_d, counts_d = torch.from_numpy(rows).to(dev), torch.from_numpy(counts).to(dev)
    r1, c1 = rows_d[:K].contiguous(), counts_d[:K].contiguous()
    pred = torch.empty((1, 4 + NC, K * MAX_DET), dtype=torch.float32, device=dev)
    nbufs = H.NmsBuffers(1, K * MAX_DET, KEEP, dev)

    def parent():
        H.check(lib().dy_rows_to_pred(r1.data_ptr(), c1.data_ptr(), offs_d.data_ptr(), pred.data_ptr(), K, MAX_DET, NC, st()))
        H.nms(pred, 0.0, THR, max_det=KEEP, nc=NC, bufs=nbufs)

    one = lambda: H.tile_merge((r1, c1), offs_d, K, (HF, WF), NC, THR, 0, False, KEEP)  # noqa: E731
    eight = lambda: H.tile_merge((rows_d, counts_d), offs_d, K, (HF, WF), NC, THR, 0, False, KEEP)  # noqa: E731
    fuse = lambda r, c, mode: lambda: H.tile_merge((r, c), offs_d, K, (HF, WF), NC, THR, 0, False, KEEP, mode=mode)  # noqa: E731
    fns = {"parent": parent, "tile_merge": one, "tile_merge_x8": eight, "union": fuse(r1, c1, "union"), "wbf": fuse(r1, c1, "wbf"),
           "union_x8": fuse(rows_d, counts_d, "union"), "wbf_x8": fuse(rows_d, counts_d, "wbf")}
    if a.obb:  # the same objects as x, y, w, h, theta, conf, cls: the angle of a row follows its score, so the views of an object share it
        x1, y1, x2, y2, sc, cl = rows_d.unbind(2)
        rrows_d = torch.stack(((x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1, sc.round(decimals=1) * 1.5, sc, cl), 2).contiguous()
        rr1 = rrows_d[:K].contiguous()
        fns["rotated"] = lambda: H.tile_merge_rotated((rr1, c1), offs_d, K, (HF, WF), NC, THR, False, KEEP)  # noqa: E731
        fns["rotated_x8"] = lambda: H.tile_merge_rotated((rrows_d, counts_d), offs_d, K, (HF, WF), NC, THR, False, KEEP)  # noqa: E731
    ts = ab(fns, a.rounds)
    same = bool(torch.equal(nbufs.index[0, : int(nbufs.count[0])], one().index[0, : int(nbufs.count[0])])) and int(nbufs.count[0]) == int(one().count[0])
    kept = one().index[0].clone()
    fused = fuse(r1, c1, "union")()
    same_fused = bool(torch.equal(fused.index[0], kept))
    out["merge"].append({"rows_per_tile": round(float(counts[:K].mean()), 1), "kept": int(nbufs.count[0]), "same_rows_kept": same,
                         "fuse_keeps_the_same_rows": same_fused, "absorbed": int((fused.members[0] - 1).clamp(min=0).sum()),
                         "parent_rows_to_pred_nms_ms": stat(ts["parent"]), "tile_merge_ms": stat(ts["tile_merge"]),
                         "tile_merge_8_frames_ms_per_frame": stat([t / 8 for t in ts["tile_merge_x8"]]),
                         "tile_fuse_union_ms": stat(ts["union"]), "tile_fuse_wbf_ms": stat(ts["wbf"]),
                         "tile_fuse_union_8_frames_ms_per_frame": stat([t / 8 for t in ts["union_x8"]]),
                         "tile_fuse_wbf_8_frames_ms_per_frame": stat([t / 8 for t in ts["wbf_x8"]])})
    if a.obb:
        out["merge"][-1].update({"tile_merge_rotated_ms": stat(ts["rotated"]), "tile_merge_rotated_8_frames_ms_per_frame": stat([t / 8 for t in ts["rotated_x8"]]),
                                 "rotated_kept": int(fns["rotated"]().count[0])})
    print(json.dumps(out["merge"][-1]), file=sys.stderr, flush=True)

# ---- (b) the slicer ---------------------------------------------------------------------------------------------------------------------------
frames8 = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (8, HF, WF, 3), dtype=np.uint8)).to(dev)
tiles8 = torch.empty((8 * K, 3, a.tile, a.tile), dtype=torch.float32, device=dev)
tv = tiles8.view(8, K, 3, a.tile, a.tile)


def single8():
    for f in range(8):
        H.check(lib().dy_tiles_u8_to_nchw_f32(frames8[f].data_ptr(), offs_d.data_ptr(), tv[f].data_ptr(), K, HF, WF, a.tile, a.tile, 1, 114.0, st()))


ts = ab({"single": single8, "batched": lambda: H.tiles_batch(frames8, offs_d, a.tile, out=tiles8)}, a.rounds)
gb = tiles8.numel() * 4 / 1e9
out["slicer"] = {"frames": 8, "written_GB": round(gb, 3), "eight_single_launches_ms": stat(ts["single"]), "one_batched_launch_ms": stat(ts["batched"]),
                 "single_GBps": round(gb / np.median(ts["single"]) * 1e3, 1), "batched_GBps": round(gb / np.median(ts["batched"]) * 1e3, 1)}
print(json.dumps(out["slicer"]), file=sys.stderr, flush=True)
del tiles8, tv

# ---- (c) frames per second end to end ----------------------------------------------------------------------------------------------------------
if not a.no_e2e:
    from drone_yolo_amd.utils.parity import seeded_state_dict

    yolo = D.YOLO(f"yolov8{a.scale}-p2-repvgg{'-obb' if a.obb else ''}.yaml")
    yolo.model.load_state_dict(seeded_state_dict(yolo.model.state_dict(), 5, cls_bias=-1.2))
    video = [np.ascontiguousarray(f) for f in np.random.default_rng(2).integers(0, 256, (a.frames, HF, WF, 3), dtype=np.uint8)]
    common = dict(conf=0.25, iou=0.7, dtype=a.dtype, device=0)
    tp = None if a.obb else TiledPredictor(yolo.model, tile=a.tile, overlap=a.overlap, merge_iou=THR, merge_max_det=KEEP, **common)

    def per_frame():
        return [len(tp(f)) for f in video]

    def batched(F):
        return [len(r) for r in yolo.predict(video, tile=a.tile, tile_overlap=a.overlap, merge_iou=THR, merge_max_det=KEEP, batch=F, stream=True, **common)]

    runs = {"TiledPredictor_per_frame": per_frame, "predict_batch1": lambda: batched(1), "predict_batch2": lambda: batched(2), "predict_batch4": lambda: batched(4)}
    if a.obb:
        runs.pop("TiledPredictor_per_frame")
    fps = {k: [] for k in runs}
    boxes = {}
    for k, fn in runs.items():  # warm-up: records and captures every pass
        boxes[k] = int(sum(fn()))
    rounds = max(3, a.rounds // 2)
    for _ in range(rounds):
        for k, fn in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            fps[k].append(a.frames / (time.perf_counter() - t0))
    out["end_to_end"] = {"frames": a.frames, "scale": a.scale, "obb": a.obb, "dtype": a.dtype, "rounds": rounds, "boxes": boxes, "frames_per_s": {k: stat(v) for k, v in fps.items()}}
print(json.dumps(out))
