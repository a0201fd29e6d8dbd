"""GPU: training a segmentation model -- ``SegmentationModel.forward_train`` + ``v8SegmentationLoss`` + backward, the trainer's eager and
graphed steps, and ``YOLO(<-seg>).train`` end to end.

One step against the reference (tests/golden/seg_train.npz, tools/make_seg_loss_golden.py --train): the REAL reference's training-mode
SegmentationModel step on this project's -seg YAMLs (n, nc 10, seeded state dict, B = 2 at 64 x 96, index maps at a quarter of the image),
stored from its FLOAT64 run.  Bars: 16 x the reference's own fp32 difference from that run (``ref_err``), items with the floor of
tests/_loss_util.py, every gradient figure capped at 1e-4 (relative to the stored gradient's own maximum / to the norm).
Measured on an MI355X (fp32 storage): see MEASURED.
"""
import copy
import csv

import pytest
import torch

from tests import _loss_util as LU
from tests._seg_loss_util import train_labels
from tests._util import golden, load_yaml, meta

pytestmark = pytest.mark.gpu

GRAD_CEIL = 1e-4
MEASURED = {"st3n": (1.07e-5, 5.4e-5, 3.2e-5), "stp2n": (1.11e-5, 5.4e-5, 2.7e-5)}  # tag -> (items, worst stored gradient, worst norm) on an MI355X; bars 1.8e-4 / 7.0e-5, 1e-4, 1e-4


def _case(tag):
    from drone_yolo_amd.nn.tasks import SegmentationModel
    from oracle import drone_yolo_oracle as O

    g = golden("seg_train.npz")
    m = meta(g, tag)
    model = SegmentationModel(dict(load_yaml(m["yaml"], m["scale"], m["nc"])), nc=m["nc"], verbose=False)
    model.load_state_dict(O.seeded_state_dict(model.state_dict(), m["seed"], cls_bias=m["cls_bias"]))
    b, h, w = m["shape"]
    img = torch.randint(0, 256, (b, 3, h, w), generator=torch.Generator().manual_seed(m["seed"]), dtype=torch.uint8)
    return g, m, model, img, train_labels(m["seed"], (h, w))


@pytest.mark.parametrize("tag", ["st3n", "stp2n"])
def test_one_training_step_against_the_reference(tag, device):
    g, m, model, img, labels = _case(tag)
    e_items, e_full, e_norm = (float(x) for x in g[f"{tag}__ref_err"])
    item_bar = LU.FACTOR * max(e_items, LU.F32_EPS)
    grad_bar, norm_bar = min(GRAD_CEIL, LU.FACTOR * max(e_full, LU.F32_EPS)), min(GRAD_CEIL, LU.FACTOR * max(e_norm, LU.F32_EPS))
    model = model.to(device).train()
    model.train_dtype = torch.float32
    feats, coefs, proto = model.forward_train(img.to(device))
    ratio = 2 if len(model.stride) == 4 else 1
    assert len(feats) == len(coefs) == len(model.stride) and all(c.shape[1] == 32 and c.dtype == torch.float32 and c.shape[2:] == f.shape[2:] for f, c in zip(feats, coefs))
    assert tuple(proto.shape) == (2, 32, 16 * ratio, 24 * ratio) and proto.dtype == torch.float32
    loss, items = model(dict(img=img.to(device), **labels))
    loss.backward()
    torch.cuda.synchronize()
    ref = torch.cat((torch.from_numpy(g[f"{tag}__items"]), torch.from_numpy(g[f"{tag}__total"]).view(1)))
    got = torch.cat((items.detach().cpu().double(), loss.detach().cpu().double().view(1)))
    e_it = LU.item_err(got, ref)
    print(tag, "items (box, seg, cls, dfl), total", got.tolist(), "float64 reference", ref.tolist(), "err", e_it, "bar", item_bar)
    params = dict(model.named_parameters())
    full = [str(k) for k in g[f"{tag}__full_keys"]]
    head = len(model.model) - 1
    for k in [f"model.{head}.cv4.{lvl}.2.{p}" for lvl in range(len(model.stride)) for p in ("weight", "bias")] + [
            f"model.{head}.proto.upsample.weight", f"model.{head}.proto.upsample.bias", f"model.{head}.proto.cv3.conv.weight", f"model.{head}.proto.cv3.bn.weight"]:
        assert k in full, k
    assert any(k.startswith("model.0.") for k in full)
    worst, worst_k = 0.0, None
    for i, k in enumerate(full):
        r = torch.from_numpy(g[f"{tag}__full_{i}"])
        got_g = params[k].grad
        assert got_g is not None and tuple(got_g.shape) == tuple(r.shape), k
        e = float((got_g.cpu() - r).abs().max()) / max(float(r.abs().max()), 1e-30)
        if e > worst:
            worst, worst_k = e, k
    keys = [str(k) for k in g[f"{tag}__norm_keys"]]
    assert set(keys) | set(full) == {k for k, p in params.items() if p.requires_grad and ".dfl." not in k}
    norms = torch.tensor([float(params[k].grad.double().norm()) for k in keys], dtype=torch.float64)
    rn = torch.from_numpy(g[f"{tag}__norms"])
    en = (norms - rn).abs() / rn.clamp(min=1e-30)
    print(tag, "worst stored gradient", worst, worst_k, "bar", grad_bar, "| worst norm", float(en.max()), keys[int(en.argmax())], "bar", norm_bar)
    assert e_it <= item_bar, (e_it, item_bar)
    assert worst <= grad_bar, (worst, worst_k, grad_bar)
    assert float(en.max()) <= norm_bar, (float(en.max()), keys[int(en.argmax())], norm_bar)


def test_graphed_steps_equal_eager_steps(device):
    """The trainer's third step on replays forward + v8SegmentationLoss + backward as a hipGraph with the label table AND the index maps in
    static buffers.  Four steps with changing labels and maps (two eager, then the capture and one more replay), graphed against eager, with
    the bars and the step count of the oriented-box twin (tests/test_obb_train_gpu.py says why four steps at lr0 0.001)."""
    from drone_yolo_amd.engine.trainer import DetectionTrainer

    g, m, model, img, _ = _case("st3n")
    runs = {}
    for graphed in (False, True):
        mdl = copy.deepcopy(model)
        tr = DetectionTrainer(mdl, dict(optimizer="SGD", lr0=0.001, momentum=0.937, batch=64, dtype="fp32", warmup_epochs=0.0))
        tr.graph_steps = graphed
        losses, rows = [], []
        for it in range(4):
            loss, items = tr.step(dict(img=img.to(device), **train_labels(100 + it)), epoch=0, nb=1000)
            losses.append(float(loss.detach()))
            rows.append(items.detach().cpu())
        torch.cuda.synchronize()
        assert (getattr(tr, "_graph", None) is not None) == graphed and all(r.numel() == 4 for r in rows)
        if graphed:
            assert tuple(tr._graph["masks"].shape) == (2, 16, 24) and tr._graph["masks"].dtype == torch.uint8 and tr._graph["gt"].shape[2] == 5
            assert torch.equal(tr._graph["masks"].cpu(), train_labels(103)["masks"])  # the last step's maps reached the static buffer
        runs[graphed] = (losses, rows, {k: v.detach().float().cpu().clone() for k, v in mdl.state_dict().items()})
    for a, b in zip(runs[False][0], runs[True][0]):
        assert abs(a - b) <= 1e-3 * abs(a), (runs[False][0], runs[True][0])
    for a, b in zip(runs[False][1], runs[True][1]):
        assert torch.allclose(a, b, rtol=1e-3, atol=1e-5), (a, b)
    moved = set()
    for k, v in runs[False][2].items():
        if v.is_floating_point() and "dfl.conv" not in k:
            err = float((runs[True][2][k] - v).abs().max()) / max(float(v.abs().max()), 1e-6)
            assert err <= (5e-3 if "running_" in k else 2e-3), (k, err)
            if not torch.equal(v, model.state_dict()[k].float()):
                moved.add(k)
    assert any(".cv4." in k and k.endswith("2.weight") for k in moved), "the coefficient tails did not train"
    assert any(k.endswith("proto.upsample.weight") for k in moved) and any(k.endswith("proto.upsample.bias") for k in moved), "Proto's transposed convolution did not train"


def test_yolo_train_api_end_to_end(device, tmp_path):
    """``YOLO("yolov8n-seg.yaml").train(data="synthetic-seg:8", ...)``: two epochs; results.csv carries the four train losses and, with
    ``val="train"``, SegmentMetrics' (B) and (M) keys from the per-epoch ``SegmentationValidator``; last.pt loads back through ``YOLO(path)`` as
    task segment and predicts masks; a killed run resumes."""
    import drone_yolo_amd as D
    from drone_yolo_amd.engine.trainer import DetectionTrainer
    from drone_yolo_amd.engine.validator import SegmentationValidator
    from drone_yolo_amd.nn.tasks import SegmentationModel

    yolo = D.YOLO("yolov8n-seg.yaml")
    head = yolo.model.model[-1]
    w0, u0 = head.cv4[0][2].weight.detach().clone(), head.proto.upsample.weight.detach().clone()
    common = dict(data="synthetic-seg:8", epochs=2, imgsz=64, batch=8, nbs=8, device=0, dtype="fp32", optimizer="SGD", lr0=0.01, warmup_epochs=0.0, project=str(tmp_path),
                  val="train")
    out = yolo.train(name="t", **common)
    assert isinstance(yolo.trainer.validator, SegmentationValidator) and isinstance(yolo.trainer.model, SegmentationModel)
    assert yolo.trainer.loss_names == ("box_loss", "seg_loss", "cls_loss", "dfl_loss")
    rows = list(csv.DictReader(open(tmp_path / "t" / "results.csv")))
    assert [r["epoch"] for r in rows] == ["1", "2"]
    assert {"train/box_loss", "train/seg_loss", "train/cls_loss", "train/dfl_loss", "metrics/mAP50(B)", "metrics/mAP50-95(B)", "metrics/mAP50(M)", "metrics/mAP50-95(M)"} <= set(rows[0])
    assert not any(k.startswith("val/") for k in rows[0])
    assert all(float(r["train/cls_loss"]) > 0 and float(r["train/seg_loss"]) > 0 for r in rows) and "train/seg_loss" in out
    head = yolo.model.model[-1]
    assert not torch.equal(head.cv4[0][2].weight.detach().cpu(), w0) and not torch.equal(head.proto.upsample.weight.detach().cpu(), u0)
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(1))
    again = D.YOLO(str(tmp_path / "t" / "weights" / "last.pt"))
    assert again.task == "segment" and isinstance(again.model, SegmentationModel)
    res = again.predict(x, device=0, conf=1e-5, dtype="fp32")  # (two epochs leave the class scores near their initial prior)
    assert len(res) == 2 and sum(r.boxes.data.shape[0] for r in res) > 0
    for r in res:  # an image without detections carries no masks; otherwise one mask per box
        assert (r.masks is None) == (r.boxes.data.shape[0] == 0) and (r.masks is None or r.masks.data.shape[0] == r.boxes.data.shape[0])

    class Killed(Exception):
        pass

    class DiesAfterEpoch1(DetectionTrainer):
        def save_model(self):
            super().save_model()
            if self.epoch == 0:
                raise Killed

    victim = DiesAfterEpoch1(overrides=dict(common, model="yolov8n-seg.yaml", nc=10, name="victim"))
    with pytest.raises(Killed):
        victim.train()
    assert isinstance(victim.model, SegmentationModel)
    last = tmp_path / "victim" / "weights" / "last.pt"
    del victim
    resumed = DetectionTrainer(overrides=dict(resume=str(last), data="synthetic-seg:8"))
    resumed.train()
    assert resumed.start_epoch == 1 and resumed.epoch == 1 and isinstance(resumed.model, SegmentationModel)
    assert resumed.read_results_csv()["epoch"] == [1.0, 2.0]


def test_one_rank_rccl_group_trains_a_seg_model(device, tmp_path):
    """The multi-rank path with a segmentation model, by tests/test_train_gpu.py's one-rank RCCL pattern: ONE rank started as a child process
    (backend nccl, DYOLO_DDP_SINGLE_RANK=1), gradient buckets armed, the graphed step cut behind each bucket's flush.  A SUM over one rank is
    the identity: the parameters after five steps equal the same trainer's without a process group up to the order of fp32 sums."""
    import os

    from drone_yolo_amd.utils.dist import launch_ranks
    from tests._ddp_seg_train_worker import run_steps

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "rccl_seg.pt"
    rc = launch_ranks(1, os.path.join(root, "tests", "_ddp_seg_train_worker.py"), [str(out)],
                      env={"DYOLO_DDP_SINGLE_RANK": "1", "DYOLO_TRAIN_GRAPH": "1", "DYOLO_DDP_GRAPH_CUT": "1", "DYOLO_DIST_BACKEND": None, "DYOLO_FORCE_DEVICE": None})
    assert rc == 0, f"one-rank RCCL run exited with {rc}"
    o = torch.load(out, weights_only=False)
    assert o["backend"] == "nccl" and o["world"] == 1 and o["graphs"] == o["buckets"] >= 2 and o["masks"] == (2, 16, 24), o
    tr = run_steps(device)
    assert tr.buckets is None
    ref = tr.flat.P.cpu()
    for k, (off, c) in tr.flat.offsets.items():
        a, b = o["P"][off : off + c], ref[off : off + c]
        assert float((a - b).abs().max()) <= 2e-3 * max(float(b.abs().max()), 1e-3), k
