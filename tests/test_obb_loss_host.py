"""CPU: the oriented-box loss sweep (tests/_obb_loss_util.py) is sound, and its bars have teeth.

* ``v8OBBLoss.targets_to_gt`` / ``preprocess`` build the rows the real reference builds (tests/golden/obb_loss.npz) on ``tiny``, ``negsum``
  and an empty batch: the tiny-box filter with the width times the image HEIGHT, the six columns, and -- the one deliberate difference --
  the rows the reference masks by ``x + y + w + h + r <= 0`` are dropped on the host instead of being carried as padding;
* the float64 restatement reproduces the real reference's fp32 run on every case: same owners outside the unsure set, items and gradients
  within the detection loss's ceilings;
* MEASURED_PAIR_ERR covers the reference's fp32 distance from float64 on every in-box pair; the unsure set is empty in every case but
  ``edge`` (tests/_obb_loss_util.py says why), where only kind (c) is populated -- under the float64 inequalities; with membership pinned
  by the fp32 restatement of the kernel's in-box arithmetic (which equals the reference's mask on every case) it is empty in ``edge`` too
  and the owner map equals the real reference's at every anchor of every case;
* every case holds the geometry it was built for;
* each mutant of the restatement, fed to the SAME ``check_case`` the GPU test uses, fails on the cases named in CATCHERS.
"""
import math

import numpy as np
import pytest
import torch

from tests import _obb_loss_util as U

# mutant -> the cases that must catch it, and by which check (o = owner map, i = items, g = gradient)
CATCHERS = {
    "inbox_strict": [("edge", "o")],
    "w_times_w": [("tiny", "o")],
    "dfl_rotated_target": [("rand", "ig"), ("thin", "ig")],
    "overlap_unclamped": [("clampov", "o")],
    "pixel_units_in_loss": [("tiny", "i")],
    "angle_centre_route_dropped": [("rand", "g"), ("conv", "g")],
    "mask_gt_on_xywh": [("negsum", "o")],
    "last_tie": [("dup", "o")],
    "topk_minus_1": [("rand", "o"), ("conv", "o")],
}


def _criterion(nc=10, strides=U.S3):
    from drone_yolo_amd.utils.loss import v8OBBLoss

    crit = object.__new__(v8OBBLoss)
    crit.nc, crit.reg_max, crit.stride, crit.topk, crit.box, crit.cls, crit.dfl = nc, 16, torch.tensor(strides), 10, 7.5, 0.5, 1.5
    return crit


@pytest.mark.parametrize("cid", ["tiny", "negsum", "none"])
def test_label_table_rows_equal_the_reference(cid):
    case, g32 = U.build_case(cid), U.golden(cid)
    ref = g32["gt"]
    assert torch.equal(U.table_from_labels(case["labels"], 2, case["hw"]), ref)  # the restatement's table is the reference's, bit for bit
    gt = _criterion().targets_to_gt(case["labels"], 2, case["hw"])
    assert gt.dtype == torch.float32 and gt.shape[0] == 2 and gt.shape[2] == 6
    for b in range(2):
        live = ref[b][ref[b, :, 1:].sum(-1) > 0]  # mask_gt: what the reference's assigner sees
        ours = gt[b][gt[b].abs().sum(-1) > 0]
        assert torch.equal(ours, live), (cid, b, ours, live)
    if cid == "tiny":
        kept = [r for r, k in U.TINY_ROWS if k]
        assert ref.shape[1] == len(kept) == 3 and ref[0, :, 0].tolist() == [float(r[0]) for r in kept]
        W, H = np.float32(96), np.float32(64)  # the two rows the h / w exchange decides
        assert np.float32(2.5) / W * H < 2 <= np.float32(2.5) and np.float32(1.5) < 2 <= np.float32(1.5) / H * W
    if cid == "negsum":
        assert ref.shape[1] == 2 and float(ref[0, 0, 1:].sum()) <= 0 < float(ref[0, 0, 1:5].sum())  # carried by the reference, masked by its sum
        assert gt.shape[1] == 1 and gt[0, 0, 0] == 5  # dropped here
    if cid == "none":
        assert tuple(gt.shape) == (2, 0, 6) and tuple(ref.shape) == (2, 0, 6)


def test_four_column_labels_are_refused_by_the_criterion():
    batch = {"batch_idx": torch.zeros(2), "cls": torch.zeros(2, 1), "bboxes": torch.rand(2, 4)}
    with pytest.raises(TypeError, match=r"\(M, 5\) xywhr"):
        _criterion().targets_to_gt(batch, 2, U.HW)
    bad = {"batch_idx": torch.zeros(1), "cls": torch.full((1, 1), 10.0), "bboxes": torch.tensor([[0.5, 0.5, 0.3, 0.3, 0.1]])}
    with pytest.raises(ValueError, match=r"class outside \[0, 10\)"):
        _criterion().targets_to_gt(bad, 2, U.HW)


@pytest.mark.parametrize("cid", U.CASE_IDS)
def test_restatement_reproduces_the_reference(cid):
    case, asg, g32, bars = U.case_reference(cid)
    assert torch.equal(g32["gt"], case["gt"])
    assert asg["kinds"] == (0, 0, 0) and not bool(asg["unsure"].any()), f"{cid}: unsure anchors {asg['kinds']}: pick other seeds (tools/make_obb_loss_golden.py --seeds)"
    # membership: the fp32 restatement of the kernel's arithmetic is the reference's own mask (its overlaps are written inside the mask only;
    # clampov's three zero-size predictions have overlap 0 inside it), and with it the owner map is the reference's at EVERY anchor
    mask = U.inbox32(case["feats"], case["gt"], case["strides"])
    if case["gt"].shape[1]:
        diff = mask != (g32["overlap"] > 0)
        assert int(diff.sum()) == (3 if cid == "clampov" else 0) and bool(mask[diff].all())
    assert torch.equal(asg["inbox"], mask) and torch.equal(g32["owner"], asg["owner"]), f"{cid}: owners differ from the reference at {(g32['owner'] != asg['owner']).nonzero().tolist()}"
    free = U.assign64_rot(case["feats"], case["angles"], case["gt"], case["strides"], case["nc"], case["topk"])  # the float64 inequalities alone
    assert free["kinds"][:2] == (0, 0) and (free["kinds"][2] > 0) == (cid == "edge"), (cid, free["kinds"])
    if cid == "edge":  # what float64 cannot decide, fp32 does: r = 0 is exact in both; the r = pi/2 image is where they part
        assert free["kinds"][2] == 27 and not bool(free["unsure"][0].any()) and int((free["inbox"] != mask).sum()) == 11 and torch.equal(free["inbox"][0], mask[0])
        assert int((free["owner"] != g32["owner"]).sum()) == 6
    extra = g32["fg"] & (g32["owner"] < 0)
    assert bool((g32["tscore"][extra] == 0).all())  # the reference's zero-metric picks: foreground with target score 0
    print(cid, {k: bars[k] for k in ("oracle_items", "oracle_grad", "items", "grad")}, "fg", int((asg["owner"] >= 0).sum()), "pair", U.pair_err(cid))
    assert bars["oracle_items"] <= U.ITEM_CEIL and bars["oracle_grad"] <= U.GRAD_CEIL, bars
    res = U.check_case(cid, g32["owner"], torch.cat((g32["items"], g32["total"].view(1))), g32["grads"], g32["agrads"])
    assert res["ok"], res


def test_delta_covers_the_reference_in_fp32():
    worst = 0.0
    for cid in U.CASE_IDS:
        e = U.pair_err(cid)
        assert e <= U.MEASURED_PAIR_ERR, f"{cid}: the fp32 reference is {e:.2e} from float64 on a pair, above the figure DELTA rests on"
        worst = max(worst, e)
    print("largest pair error", worst, "DELTA", U.DELTA)
    assert worst >= U.MEASURED_PAIR_ERR / 4, "MEASURED_PAIR_ERR no longer describes the sweep: measure it again"
    assert U.DELTA == 16 * U.MEASURED_PAIR_ERR


def test_cases_hold_the_geometry_they_were_built_for():
    n_in = lambda cid: U.case_reference(cid)[1]["inbox"].sum(-1)  # noqa: E731
    # edge, r = 0: x 12..60 holds the stride-8 columns 1..7, y 20..36 the rows 2..4, edges included; strict inequalities leave 5 x 1
    _, asg, g32, _ = U.case_reference("edge")
    s8 = asg["inbox"][0, 0, :96].reshape(8, 12)
    assert int(s8.sum()) == 7 * 3 and bool(s8[2:5, 1:8].all())
    assert torch.equal(g32["overlap"][0, 0, :96].reshape(8, 12) > 0, s8) or int((g32["overlap"][0, 0, :96] > 0).sum()) <= 21
    strict = U.assign64_rot(*[U.build_case("edge")[k] for k in ("feats", "angles", "gt", "strides", "nc")], mut=("inbox_strict",))["inbox"][0, 0, :96]
    assert int(strict.sum()) == 5 * 1
    # thin: 3 x 60 boxes at 45 degrees hold a handful of anchors of a hull of hundreds of square pixels
    t = n_in("thin")
    assert bool((t > 0).all()) and bool((t <= 12).all()), t
    # dup: identical rows go to the first index; the crossed pair shares anchors about its centre
    _, asg, _, _ = U.case_reference("dup")
    assert int((asg["owner"][0] == 0).sum()) > 0 and int((asg["owner"][0] == 1).sum()) == 0
    shared = asg["claims"][1] > 1  # image 1: one rectangle under two classes: what both pick goes to the first
    assert int(shared.sum()) > 0 and bool((asg["owner"][1][shared] == 0).all())
    assert int((asg["inbox"][0, 2] & asg["inbox"][0, 3]).sum()) > 0 and int((asg["claims"][0] > 1).sum()) > 0
    # crowd: 40 labels on image 0, none on image 1
    case, asg, _, _ = U.case_reference("crowd")
    assert case["gt"].shape[1] == 40 and not bool(case["gt"][1].any()) and bool((asg["owner"][1] < 0).all()) and int(asg["claims"][0].max()) >= 3
    # none
    case, asg, g32, _ = U.case_reference("none")
    assert case["gt"].shape == (2, 0, 6) and float(g32["items"][0]) == 0 and float(g32["items"][2]) == 0
    assert all(not bool(g.any()) for g in g32["agrads"]) and all(bool(g[:, 64:].all()) for g in g32["grads"])
    # negsum: the masked label holds an anchor, and owns none
    case, asg, _, _ = U.case_reference("negsum")
    assert float(case["gt"][0, 0, 1:].sum()) <= 0 and int((asg["owner"][0] == 0).sum()) == 0 and int((asg["owner"][0] == 1).sum()) > 0
    free = U.assign64_rot(*[case[k] for k in ("feats", "angles", "gt", "strides", "nc")], mut=("mask_gt_on_xywh",))
    assert int(free["inbox"][0, 0].sum()) >= 1
    # wrap: the three angles of the regularisation fixtures
    r = U.build_case("wrap")["gt"][..., 5]
    assert float(r[0, 0]) == -U.PI32 / 4 and float(r[0, 1]) < 0.75 * math.pi and float(r[1, 0]) == U.PI32 / 2
    # nc1 / nc80: both ends of the class range are owned
    for nc in (1, 80):
        case, asg, _, _ = U.case_reference(f"nc{nc}")
        bi, ai = (asg["owner"] >= 0).nonzero(as_tuple=True)
        assert set(case["gt"][bi, asg["owner"][bi, ai], 0].long().tolist()) == {0, nc - 1}
    # pad: more padding rows than labels, in the middle of the table too; an image without labels; the table goes to the device as it is
    case = U.build_case("pad")
    live = case["gt"][1, :, 1:].sum(-1) > 0
    assert case["device_table"] and not bool(case["gt"][0].any()) and int(live.sum()) == 5 and case["gt"].shape[1] == 14 and not bool(live[0]) and bool(live[1])
    # conv: the P2 stride set, converged heads
    case, asg, _, _ = U.case_reference("conv")
    info = U.loss_from_owner64_rot(case["feats"], case["angles"], case["gt"], asg["owner"], case["strides"], case["nc"], want_grad=False)[4]
    assert [tuple(f.shape[2:]) for f in case["feats"]] == [(16, 24), (8, 12), (4, 6), (2, 3)] and info["mean_iou"] >= 0.6, info
    # big: one label holds more candidates than the pick kernel keeps in LDS (kPickCache = 1024 in csrc/obb_loss.hip), the others far fewer
    b = n_in("big")
    assert int(b[0, 0]) > 1024 and int(b[0, 1:].max()) < 1024 and int(b[1].max()) < 1024, b
    # clampov: the zero-size predictions are inside the label, and their unclamped overlap is negative
    case, asg, _, _ = U.case_reference("clampov")
    p = U._pairs(case["feats"], case["angles"], case["gt"], case["strides"], case["nc"], mut=("overlap_unclamped",))
    col = [y * 12 for y in (1, 4, 6)]
    assert bool(asg["inbox"][0, 0, col].all()) and bool((p["raw_overlap"][0, 0, col] < 0).all()) and bool((asg["owner"][0, col] < 0).all())
    assert int(asg["inbox"][0, 0].sum()) == 8


@pytest.mark.parametrize("mut", U.MUTANTS)
def test_the_bars_catch(mut):
    assert set(CATCHERS) == set(U.MUTANTS)
    for cid, how in CATCHERS[mut]:
        res = U.check_case(cid, *U.mutant_result(cid, mut))
        failed = "".join(c for c, k in (("o", "ok_owner"), ("i", "ok_items"), ("g", "ok_grad")) if not res[k])
        print(mut, cid, failed, {k: res[k] for k in ("owner_wrong", "items_err", "items_bar", "grad_err", "grad_bar")})
        assert set(how) <= set(failed), f"mutant {mut} passes {set(how) - set(failed)} of {cid}: {res}"


def test_clean_restatement_passes_every_check():
    for cid in U.CASE_IDS:
        case, asg, _, _ = U.case_reference(cid)
        items, total, grads, agrads, _ = U.loss_from_owner64_rot(case["feats"], case["angles"], case["gt"], asg["owner"], case["strides"], case["nc"], want_grad=case["grad"])
        f32 = lambda gs: [g.float() for g in gs] if gs else None  # noqa: E731
        res = U.check_case(cid, asg["owner"], torch.cat((items, total.view(1))).float(), f32(grads), f32(agrads))
        assert res["ok"], (cid, res)


def test_synthetic_obb_dataset_has_five_column_boxes():
    from drone_yolo_amd.engine.trainer import load_dataset

    d, plain = load_dataset("synthetic-obb:4", 64, 10, 0), load_dataset("synthetic:4", 64, 10, 0)
    assert d["img"].shape == (4, 3, 64, 64) and d["bboxes"].dim() == 2 and d["bboxes"].shape[1] == 5 and plain["bboxes"].shape[1] == 4
    assert torch.equal(d["img"], plain["img"]) and torch.equal(d["bboxes"][:, :4], plain["bboxes"]) and torch.equal(d["cls"], plain["cls"])  # synthetic's draws, the angle drawn after
    r = d["bboxes"][:, 4]
    assert float(r.min()) >= -math.pi / 4 and float(r.max()) < 3 * math.pi / 4 and float(r.std()) > 0.5


def test_train_refusals_come_before_any_device_use(tmp_path):
    from drone_yolo_amd import YOLO

    y = YOLO("yolov8n-obb.yaml")
    four = dict(img=torch.zeros((2, 3, 64, 64), dtype=torch.uint8), batch_idx=torch.tensor([0.0, 1.0]), cls=torch.zeros((2, 1)),
                bboxes=torch.tensor([[0.5, 0.5, 0.2, 0.2], [0.4, 0.4, 0.1, 0.3]]))
    torch.save(four, tmp_path / "four.pt")  # a .pt file is read on the host for its boxes
    five = dict(four, bboxes=torch.cat((four["bboxes"], torch.tensor([[0.3], [1.2]])), 1))
    torch.save(five, tmp_path / "five.pt")
    from drone_yolo_amd.engine.trainer import check_obb_train_data

    check_obb_train_data(str(tmp_path / "five.pt"), {}), check_obb_train_data(five, {}), check_obb_train_data("synthetic-obb:4", {})  # accepted
    for data in (four, "synthetic:4", str(tmp_path / "four.pt"), tmp_path / "four.pt"):
        with pytest.raises(NotImplementedError, match=r"train: an oriented-box model needs .*\(M, 5\) xywhr"):
            y.train(data=data, device=0)
    with pytest.raises(NotImplementedError, match="device_augment"):
        y.train(data="synthetic-obb:4", device_augment=True, device=0)
    (tmp_path / "images" / "train").mkdir(parents=True)
    (tmp_path / "labels" / "train").mkdir(parents=True)
    (tmp_path / "labels" / "train" / "a.txt").write_text("0 0.1 0.1 0.4 0.1 0.4 0.3 0.1 0.3\n")  # cls x1 y1 x2 y2 x3 y3 x4 y4
    (tmp_path / "d.yaml").write_text(f"path: {tmp_path}\ntrain: images/train\nval: images/train\nnames: [a]\n")
    with pytest.raises(NotImplementedError, match=r"data=.*corner rows"):
        y.train(data=str(tmp_path / "d.yaml"), device=0)
    assert y.trainer is None and y.predictor is None and all(p.device.type == "cpu" for p in y.model.parameters())
    with pytest.raises(NotImplementedError, match="device only"):
        y.model.init_criterion()  # the criterion is a device loss: nothing to build for a model on the CPU
    y.model.train()
    with pytest.raises(NotImplementedError, match="forward_train"):
        y.model.model[-1]([torch.zeros(1, 64, 8, 8)] * 3)
