"""GPU: training an oriented-box model -- ``OBBModel.forward_train`` + ``v8OBBLoss`` + backward, the trainer's eager and graphed steps, and
``YOLO(<-obb>).train`` end to end.

One step against the reference (tests/golden/obb_train.npz, tools/make_obb_loss_golden.py --train): the REAL reference's training-mode
OBBModel step on this project's -obb YAMLs (n, nc 10, seeded state dict, B = 2 at 64 x 96, fp32).  The bars are those of
tests/test_train_gpu.py::test_model_train_step_gradients_fp32 (items 5e-4, every stored gradient within 2e-3 of its own maximum, norms 2e-3:
fp32 MFMA sums in another order, atomics); the fixture stores the reference's own fp32-vs-float64 differences, and the test checks that
eight times those stay inside the bars (measured: items 5.5e-6, gradients 8.3e-5, norms 3.0e-5).  A seed was accepted only if the
reference's fp32 and float64 runs gave the same owner map.
"""
import copy
import csv

import pytest
import torch

from tests._obb_loss_util import _labels_from_rows, _rand_rboxes
from tests._util import golden, load_yaml, meta

pytestmark = pytest.mark.gpu

ITEM_TOL, GRAD_TOL, NORM_TOL = 5e-4, 2e-3, 2e-3


def _labels(seed, hw=(64, 96)):
    return _labels_from_rows([_rand_rboxes(seed, 4, 10, hw), _rand_rboxes(seed + 1, 3, 10, hw)], hw)


def _case(tag):
    from drone_yolo_amd.nn.tasks import OBBModel
    from oracle import drone_yolo_oracle as O

    g = golden("obb_train.npz")
    m = meta(g, tag)
    model = OBBModel(dict(load_yaml(m["yaml"], m["scale"], m["nc"])), nc=m["nc"], verbose=False)
    model.load_state_dict(O.seeded_state_dict(model.state_dict(), m["seed"], cls_bias=m["cls_bias"]))
    b, h, w = m["shape"]
    img = torch.randint(0, 256, (b, 3, h, w), generator=torch.Generator().manual_seed(m["seed"]), dtype=torch.uint8)
    return g, m, model, img, _labels(m["seed"], (h, w))


@pytest.mark.parametrize("tag", ["ot3n", "otp2n"])
def test_one_training_step_against_the_reference(tag, device):
    g, m, model, img, labels = _case(tag)
    e_items, e_full, e_norm = (float(x) for x in g[f"{tag}__ref_err"])
    assert 8 * e_items <= ITEM_TOL and 8 * e_full <= GRAD_TOL and 8 * e_norm <= NORM_TOL  # the bars leave room for the reference's own fp32 noise
    model = model.to(device).train()
    model.train_dtype = torch.float32
    feats, angles = model.forward_train(img.to(device))
    assert len(feats) == len(angles) == len(model.stride) and all(a.shape[1] == 1 and a.dtype == torch.float32 and a.shape[2:] == f.shape[2:] for f, a in zip(feats, angles))
    loss, items = model(dict(img=img.to(device), **labels))
    loss.backward()
    torch.cuda.synchronize()
    total_ref, items_ref = float(g[f"{tag}__total"]), torch.from_numpy(g[f"{tag}__items"])
    print(tag, "items", items.cpu().tolist(), "reference", items_ref.tolist())
    assert abs(float(loss.detach()) - total_ref) <= ITEM_TOL * abs(total_ref), (float(loss.detach()), total_ref)
    assert torch.allclose(items.cpu(), items_ref, rtol=ITEM_TOL, atol=1e-5), (items.cpu(), items_ref)
    params = dict(model.named_parameters())
    worst, worst_k = 0.0, None
    full = [str(k) for k in g[f"{tag}__full_keys"]]
    head = len(model.model) - 1
    for lvl in range(len(model.stride)):  # the three tails of every level, the cv4 trunks and layer 0 are among them
        for k in (f"model.{head}.cv2.{lvl}.2.weight", f"model.{head}.cv3.{lvl}.2.bias", f"model.{head}.cv4.{lvl}.2.weight", f"model.{head}.cv4.{lvl}.2.bias",
                  f"model.{head}.cv4.{lvl}.0.conv.weight", f"model.{head}.cv4.{lvl}.1.bn.weight"):
            assert k in full, k
    assert any(k.startswith("model.0.") for k in full)
    for i, k in enumerate(full):
        ref = torch.from_numpy(g[f"{tag}__full_{i}"])
        got = params[k].grad
        assert got is not None and tuple(got.shape) == tuple(ref.shape), k
        e = float((got.cpu() - ref).abs().max()) / max(float(ref.abs().max()), 1e-9)
        if e > worst:
            worst, worst_k = e, k
    print(tag, "worst stored gradient", worst, worst_k)
    assert worst <= GRAD_TOL, (worst, worst_k)
    keys = [str(k) for k in g[f"{tag}__norm_keys"]]
    assert set(keys) | set(full) == {k for k, p in params.items() if p.requires_grad and ".dfl." not in k}
    norms = torch.tensor([float(params[k].grad.double().norm()) for k in keys], dtype=torch.float64)
    assert torch.allclose(norms, torch.from_numpy(g[f"{tag}__norms"]), rtol=NORM_TOL, atol=1e-7)


def test_graphed_steps_equal_eager_steps(device):
    """The trainer's third step on replays forward + v8OBBLoss + backward as a hipGraph with a static six-column label table.  Four steps
    with changing labels (two eager, then the capture and one more replay), graphed against eager, with the bars of tests/test_train_gpu.py's
    detection twin.  What the run may compare is bounded by the fixture, not by the path: on this B = 2 model two runs of the SAME path differ
    from the order of fp32 atomics alone -- measured on an MI355X, two eager and two graphed runs each: second to fourth step's loss within
    1.4e-5 of each other at lr0 0.001 (1.1e-4 at lr0 0.01), but the fifth step's labels meet a top-k near-tie that falls either way
    (104.91 / 104.91 eager, 107.44 / 104.91 graphed; at lr0 0.01 83.38 / 83.31 eager, 83.34 / 83.31 graphed), so a fifth step says nothing
    about replaying.  Hence lr0 0.001 and four steps: the property checked is that replaying changes nothing."""
    from drone_yolo_amd.engine.trainer import DetectionTrainer

    g, m, model, img, _ = _case("ot3n")
    runs = {}
    for graphed in (False, True):
        mdl = copy.deepcopy(model)
        tr = DetectionTrainer(mdl, dict(optimizer="SGD", lr0=0.001, momentum=0.937, batch=64, dtype="fp32", warmup_epochs=0.0))
        tr.graph_steps = graphed
        losses = []
        for it in range(4):
            loss, _ = tr.step(dict(img=img.to(device), **_labels(100 + it)), epoch=0, nb=1000)
            losses.append(float(loss.detach()))
        torch.cuda.synchronize()
        assert (getattr(tr, "_graph", None) is not None) == graphed
        if graphed:
            assert tr._graph["gt"].shape[2] == 6 and tr._graph["gt_ring"]["tables"][0].shape[2] == 6
        runs[graphed] = (losses, {k: v.detach().float().cpu().clone() for k, v in mdl.state_dict().items()})
    for a, b in zip(runs[False][0], runs[True][0]):
        assert abs(a - b) <= 1e-3 * abs(a), (runs[False][0], runs[True][0])
    moved = False
    for k, v in runs[False][1].items():
        if v.is_floating_point() and "dfl.conv" not in k:
            err = float((runs[True][1][k] - v).abs().max()) / max(float(v.abs().max()), 1e-6)
            assert err <= (5e-3 if "running_" in k else 2e-3), (k, err)
            if ".cv4." in k and k.endswith("2.weight"):
                moved |= not torch.equal(v, model.state_dict()[k].float())
    assert moved, "the angle tail's weights did not train"


def test_yolo_train_api_end_to_end(device, tmp_path):
    """``YOLO("yolov8n-obb.yaml").train(data="synthetic-obb:16", ...)``: two epochs; results.csv carries OBBMetrics' (B) keys from the
    per-epoch ``OBBValidator``; last.pt / best.pt load back through ``YOLO(path)`` as task obb and predict; a killed run resumes."""
    import drone_yolo_amd as D
    from drone_yolo_amd.engine.trainer import DetectionTrainer
    from drone_yolo_amd.engine.validator import OBBValidator
    from drone_yolo_amd.nn.tasks import OBBModel

    yolo = D.YOLO("yolov8n-obb.yaml")
    w0 = yolo.model.model[-1].cv4[0][2].weight.detach().clone()
    common = dict(data="synthetic-obb:16", epochs=2, imgsz=64, batch=8, nbs=8, device=0, dtype="fp32", optimizer="SGD", lr0=0.01, warmup_epochs=0.0, project=str(tmp_path),
                  val="train")
    out = yolo.train(name="t", **common)
    assert isinstance(yolo.trainer.validator, OBBValidator) and isinstance(yolo.trainer.model, OBBModel) and yolo.trainer.model.criterion.width == 6
    rows = list(csv.DictReader(open(tmp_path / "t" / "results.csv")))
    assert [r["epoch"] for r in rows] == ["1", "2"]
    assert {"train/box_loss", "train/cls_loss", "train/dfl_loss", "metrics/precision(B)", "metrics/recall(B)", "metrics/mAP50(B)", "metrics/mAP50-95(B)"} <= set(rows[0])
    assert all(float(r["train/cls_loss"]) > 0 for r in rows) and "train/box_loss" in out
    assert not torch.equal(yolo.model.model[-1].cv4[0][2].weight.detach().cpu(), w0)  # the angle branch trained
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(1))
    for name in ("last.pt", "best.pt"):
        again = D.YOLO(str(tmp_path / "t" / "weights" / name))
        assert again.task == "obb" and isinstance(again.model, OBBModel)
        res = again.predict(x, device=0, conf=0.001, dtype="fp32")
        assert len(res) == 2 and res[0].obb is not None and res[0].obb.data.shape[1] == 7

    class Killed(Exception):
        pass

    class DiesAfterEpoch1(DetectionTrainer):
        def save_model(self):
            super().save_model()
            if self.epoch == 0:
                raise Killed

    victim = DiesAfterEpoch1(overrides=dict(common, model="yolov8n-obb.yaml", nc=10, name="victim"))
    with pytest.raises(Killed):
        victim.train()
    assert isinstance(victim.model, OBBModel)
    last = tmp_path / "victim" / "weights" / "last.pt"
    del victim
    resumed = DetectionTrainer(overrides=dict(resume=str(last), data="synthetic-obb:16"))
    resumed.train()
    assert resumed.start_epoch == 1 and resumed.epoch == 1 and isinstance(resumed.model, OBBModel)
    assert resumed.read_results_csv()["epoch"] == [1.0, 2.0]


def test_one_rank_rccl_group_trains_an_obb_model(device, tmp_path):
    """The multi-rank path with an oriented-box model, by tests/test_train_gpu.py's one-rank RCCL pattern: ONE rank started as a child
    process (backend nccl, DYOLO_DDP_SINGLE_RANK=1), gradient buckets armed, the graphed step cut behind each bucket's flush.  A SUM over
    one rank is the identity: the parameters after five steps equal the same trainer's without a process group up to fp32 atomics order."""
    import os

    from drone_yolo_amd.utils.dist import launch_ranks
    from tests._ddp_obb_train_worker import run_steps

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "rccl_obb.pt"
    rc = launch_ranks(1, os.path.join(root, "tests", "_ddp_obb_train_worker.py"), [str(out)],
                      env={"DYOLO_DDP_SINGLE_RANK": "1", "DYOLO_TRAIN_GRAPH": "1", "DYOLO_DDP_GRAPH_CUT": "1", "DYOLO_DIST_BACKEND": None, "DYOLO_FORCE_DEVICE": None})
    assert rc == 0, f"one-rank RCCL run exited with {rc}"
    o = torch.load(out, weights_only=False)
    assert o["backend"] == "nccl" and o["world"] == 1 and o["buckets"] == 4 and o["graphs"] == 4 and o["width"] == 6, o
    tr = run_steps(device)
    assert tr.buckets is None
    ref = tr.flat.P.cpu()
    for k, (off, c) in tr.flat.offsets.items():
        a, b = o["P"][off : off + c], ref[off : off + c]
        assert float((a - b).abs().max()) <= 2e-3 * max(float(b.abs().max()), 1e-3), k
