"""Rank program of tests/test_seg_train_gpu.py::test_one_rank_rccl_group_trains_a_seg_model (not collected): tests/_ddp_train_worker.py's
one-rank RCCL run (backend nccl, DYOLO_DDP_SINGLE_RANK=1) with a segmentation model -- the coefficient tails' and Proto's parameters land in
the gradient buckets, the graphed step (static label table and index maps) is cut behind the bucket flushes.  Rank 0 writes the parameters
and the trainer's step form to argv[1]."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from drone_yolo_amd import parallel as P  # noqa: E402
from drone_yolo_amd.engine.trainer import DetectionTrainer  # noqa: E402
from drone_yolo_amd.nn.tasks import SegmentationModel  # noqa: E402
from drone_yolo_amd.utils.parity import seeded_state_dict  # noqa: E402
from tests._seg_loss_util import train_labels  # noqa: E402


def run_steps(dev, steps=5, per_rank=2):
    model = SegmentationModel("yolov8n-seg.yaml", nc=10, verbose=False)
    model.load_state_dict(seeded_state_dict(model.state_dict(), 5, cls_bias=-1.6))
    # lr0 0.001: on a B = 2 fixture a top-k near-tie can fall either way between two runs of one path (tests/test_obb_train_gpu.py); what it
    # moves in the parameters scales with the learning rate
    tr = DetectionTrainer(model, dict(optimizer="SGD", lr0=0.001, momentum=0.9, batch=per_rank, nbs=per_rank, dtype="fp32", warmup_epochs=0.0))
    img = torch.randint(0, 256, (per_rank, 3, 64, 96), generator=torch.Generator().manual_seed(5), dtype=torch.uint8)
    for it in range(steps):
        tr.step(dict(img=img.to(dev), **train_labels(300 + it)))
    torch.cuda.synchronize()
    return tr


def main(out):
    rank, local_rank, world = P.init_distributed()
    dev = torch.device("cuda", int(os.environ.get("DYOLO_FORCE_DEVICE", local_rank)))
    torch.cuda.set_device(dev)
    tr = run_steps(dev)
    if rank == 0:
        torch.save({"P": tr.flat.P.cpu(), "step_form": tr.step_form(), "graphs": len(tr._graph["graphs"]) if getattr(tr, "_graph", None) else 0,
                    "buckets": len(tr.buckets.buckets), "world": world, "backend": torch.distributed.get_backend(), "masks": tuple(tr._graph["masks"].shape)}, out)
    torch.distributed.barrier()


if __name__ == "__main__":
    main(sys.argv[1])
