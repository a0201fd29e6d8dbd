"""CPU: the label-geometry sweep of the detection loss (tests/_loss_util.py) is sound, and its bars have teeth.

* the float64 reference reproduces the fp32 oracle on every case (same owners outside the unsure set, the oracle's extra foreground
  anchors carry target score 0, items and gradient inside today's ceilings);
* DELTA covers the fp32 oracle's distance from float64, the unsure set stays within its caps, and every condition a case was built
  for holds (converged heads have CIoU >= 0.8, the DFL clamp is hit, anchors are claimed three times, ...);
* each mutant of the reference, fed to the SAME ``check_case`` the GPU test uses, fails on the cases named in CATCHERS;
* a host box table with a class outside [0, nc) is refused before any launch.
"""
import pytest
import torch

from tests import _loss_util as U

CIOU_EXEMPT = {"sliver-C"}  # an addition to the table: 2-pixel boxes put the target 0.25 bins from the anchor, below what 16 bins resolve (0.62)

# mutant -> the cases that must catch it, and by which check (o = owner map, i = items, g = gradient)
CATCHERS = {
    "inbox_ge": [("edge-R", "oig"), ("edge-C", "oig")],
    "last_tie": [("dup-R", "o"), ("dup-C", "o"), ("ties", "o")],
    "claimants_only": [("crowd-C", "o")],
    "topk_minus_1": [("edge-C", "o"), ("ties", "o"), ("k1-R", "o")],
    "max_over_picks": [("crowd-C", "ig"), ("dup-C", "ig")],
    "no_dfl_clamp": [("clamp-C", "ig"), ("whole-C", "ig")],
    "swap_hw": [("rect-R", "oig"), ("rect-C", "oig")],
    "alpha_attached": [("edge-C", "g"), ("lv3-C", "g"), ("peak", "g")],
    "box_pixels": [("tiny", "ig")],
}


def _tied_at_boundary(asg, topk):
    """Anchors whose metric ties EXACTLY across some box's top-k boundary: torch.topk leaves their order unspecified, the kernel and the
    reference take the lowest anchor indices."""
    B, G, A = asg["metric"].shape
    tied = torch.zeros(B, A, dtype=torch.bool)
    for b in range(B):
        for g in range(G):
            r, m = asg["ranked"][b][g], asg["metric"][b, g]
            if len(r) > topk and m[r[topk - 1]] == m[r[topk]]:
                tied[b] |= m == m[r[topk]]
    return tied


@pytest.mark.parametrize("cid", U.CASE_IDS)
def test_reference_reproduces_the_float32_oracle(cid):
    case, asg, o32, bars = U.case_reference(cid)
    n_unsure = int(asg["unsure"].sum())
    assert n_unsure <= 2, f"{cid}: {n_unsure} unsure anchors: pick another head seed"
    tied = _tied_at_boundary(asg, case["topk"])
    assert bool(tied.any()) == (cid == "ties")
    diff = (asg["owner"] != o32["owner"]) & ~asg["unsure"] & ~tied
    assert not bool(diff.any()), f"{cid}: owners differ from the fp32 oracle at {diff.nonzero().tolist()}"
    extra = o32["fg"] & (o32["owner"] < 0)
    assert bool((o32["tscore"][extra] == 0).all())  # the oracle's zero-metric picks: foreground with target score 0
    assert bars["oracle_items"] <= U.ITEM_CEIL and bars["oracle_grad"] <= U.GRAD_CEIL, bars
    if not bool(tied.any()):  # the reference under its own owner map against the oracle, by the GPU test's own check
        items, total, grads, info = U.loss_from_owner64(case["feats"], case["gt"], asg["owner"], case["strides"], case["nc"], case["topk"], want_grad=case["grad"])
        res = U.check_case(cid, o32["owner"], torch.cat((o32["items"], o32["total"].view(1))), o32["grads"])
        assert res["ok"], res
        if cid.endswith("-C") and cid not in CIOU_EXEMPT:
            assert info["mean_ciou"] >= 0.8, (cid, info)
    print(cid, {k: bars[k] for k in ("oracle_items", "oracle_grad", "items", "grad")}, "fg", int((asg["owner"] >= 0).sum()))


def test_delta_covers_the_float32_oracle_and_the_unsure_set_is_small():
    worst, fg, unsure = 0.0, 0, 0
    for cid in U.CASE_IDS:
        case, asg, _, _ = U.case_reference(cid)
        e = U.pair_err(case, asg)
        assert e <= U.MEASURED_PAIR_ERR, f"{cid}: fp32 oracle is {e:.2e} from float64 on a pair, above the figure DELTA rests on"
        worst, fg, unsure = max(worst, e), fg + int((asg["owner"] >= 0).sum()), unsure + int(asg["unsure"].sum())
    print("largest pair error", worst, "DELTA", U.DELTA, "foreground", fg, "unsure", unsure)
    assert worst >= U.MEASURED_PAIR_ERR / 4, "MEASURED_PAIR_ERR no longer describes the sweep: measure it again"
    assert U.DELTA == 16 * U.MEASURED_PAIR_ERR
    assert unsure <= 0.01 * fg


def test_cases_hold_the_geometry_they_were_built_for():
    n_in = lambda cid: U.case_reference(cid)[1]["inbox"].sum(-1)  # noqa: E731  (B, G) candidates per box
    # edge: a centre ON an edge is outside (min distance 0 is not > 1e-9); one ulp inward changes nothing, one ulp outward takes the ring in
    e = n_in("edge-R")
    assert e[0].tolist() == e[1].tolist() and bool((e[2] > e[0]).all()) and bool((e[0] > 0).all()), e
    assert e[0, 0].item() == 6 * 4 + 4 * 2 + 1 + 1 and e[2, 0].item() == 8 * 6 + 4 * 2 + 1 + 1, e  # box 0: stride-4 cells 3..8 x 4..7 inside, 2..9 x 3..8 with the ring; 8 + 1 + 1 at strides 8 / 16 / 32
    # sliver: the stated number of candidates per box, and boxes with none are valid rows
    counts = n_in("sliver-R")
    assert counts[0].tolist() + counts[1, :5].tolist() == [n for _, n in U.SLIVER_ROWS], counts
    assert bool((U.build_case("sliver-R")["gt"][0, :3, 1:].sum(-1) > 0).all())
    # whole: every anchor lies in the full image and in the box past all borders; none in the boxes outside; the row whose sum is <= 0 is padding
    w = n_in("whole-R")
    assert w[0].tolist()[:3] == [340, 0, 0] and w[1].tolist()[:2] == [340, 0], w
    gt = U.build_case("whole-R")["gt"]
    assert float(gt[0, 2, 1:].sum()) <= 0 and float(gt[1, 0, 1:].sum()) > 0 and float(gt[1, 1, 1:].sum()) > 0
    # crowd: anchors claimed three times and more, and shared anchors given to a box that did not pick them
    _, asg, _, _ = U.case_reference("crowd-C")
    assert int(asg["claims"][0].max()) >= 3
    own = asg["owner"][0]
    shared = (asg["claims"][0] > 1).nonzero().flatten()
    assert any(not bool(asg["pickers"][0, int(own[a]), a]) for a in shared), "no shared anchor went to a box that had not picked it"
    # dup: identical rows go to the first index
    _, asg, _, _ = U.case_reference("dup-C")
    assert int((asg["owner"][0] == 0).sum()) > 0 and int((asg["owner"][0] == 1).sum()) == 0
    assert int((asg["owner"][2] == 0).sum()) > 0 and int((asg["owner"][2] == 4).sum()) == 0
    # pad: an image without labels, zero rows in the middle of the other's table
    gt = U.build_case("pad-R")["gt"]
    assert not bool(gt[0].any()) and not bool(gt[1, 7].any()) and bool(gt[1, 9].any()) and gt.shape[1] == 24
    assert U.build_case("gmax0-R")["gt"].shape == (2, 0, 5)
    # clamp: owned stride-4 anchors whose target passes 14.99 cells
    for cid in ("clamp-C", "whole-C"):
        case, asg, _, _ = U.case_reference(cid)
        info = U.loss_from_owner64(case["feats"], case["gt"], asg["owner"], case["strides"], case["nc"], want_grad=False)[3]
        assert info["clamp_hits"] > 0, cid
    # rect, lv3, nc: shapes and classes
    assert [tuple(f.shape[2:]) for f in U.build_case("rect-C")["feats"]] == [(16, 24), (8, 12), (4, 6), (2, 3)]
    assert len(U.build_case("lv3-C")["feats"]) == 3
    for nc in (1, 3, 80):
        case, asg, _, _ = U.case_reference(f"nc{nc}-R")
        bi, ai = (asg["owner"] >= 0).nonzero(as_tuple=True)
        owned = set(case["gt"][bi, asg["owner"][bi, ai], 0].long().tolist())
        assert owned == {0, nc - 1}, (nc, owned)
    # peak: zero-size predictions never own (their overlap clamps to 0); +-50 class logits sit on owned and background anchors alike
    case, asg, _, _ = U.case_reference("peak")
    cl = torch.cat([f.reshape(2, 74, -1) for f in case["feats"]], 2)[:, 64:]
    assert bool((cl == 50).any()) and bool((cl == -50).any())
    assert bool(((cl.amax(1) == 50) & (asg["owner"] >= 0)).any()) and bool(((cl.amax(1) == -50) & (asg["owner"] < 0)).any())
    # tiny: the one anchor of each image is owned
    _, asg, _, _ = U.case_reference("tiny")
    assert asg["owner"][:, 0].tolist() == [0, 0] and int((asg["owner"] >= 0).sum()) == 2


@pytest.mark.parametrize("mut", U.MUTANTS)
def test_the_bars_catch(mut):
    assert set(CATCHERS) == set(U.MUTANTS)
    for cid, how in CATCHERS[mut]:
        res = U.check_case(cid, *U.mutant_result(cid, mut))
        failed = "".join(c for c, k in (("o", "ok_owner"), ("i", "ok_items"), ("g", "ok_grad")) if not res[k])
        print(mut, cid, failed, {k: res[k] for k in ("owner_wrong", "items_err", "items_bar", "grad_err", "grad_bar")})
        assert set(how) <= set(failed), f"mutant {mut} passes {set(how) - set(failed)} of {cid}: {res}"


def test_clean_reference_passes_every_check():
    for cid in U.CASE_IDS:
        case, asg, _, _ = U.case_reference(cid)
        items, total, grads, _ = U.loss_from_owner64(case["feats"], case["gt"], asg["owner"], case["strides"], case["nc"], case["topk"], want_grad=case["grad"])
        res = U.check_case(cid, asg["owner"], torch.cat((items, total.view(1))).float(), [g.float() for g in grads] if grads else None)
        assert res["ok"], (cid, res)


def test_the_64_pixel_case_of_test_loss_gpu_assigns_at_least_20_anchors():
    from oracle import loss_oracle as LO

    gg = torch.Generator().manual_seed(7)
    feats = [torch.randn(2, 74, 64 // int(s), 64 // int(s), generator=gg) * 1.5 for s in U.S4]
    _, items, asg = LO.v8_detection_loss(feats, U.large_box_labels(2, 7), list(U.S4), 10, return_assign=True)
    assert int((asg["target_scores"].sum(-1) > 0).sum()) >= 20 and float(items[0]) > 1 and float(items[2]) > 1


def test_class_outside_the_head_is_refused_on_the_host():
    """``(int)g5[0]`` indexes the class logits unchecked in the kernels: a host table with such a class never reaches a launch."""
    from drone_yolo_amd.utils.loss import v8DetectionLoss

    crit = object.__new__(v8DetectionLoss)
    crit.nc, crit.reg_max, crit.stride, crit.topk, crit.box, crit.cls, crit.dfl = 10, 16, torch.tensor([4.0, 8.0, 16.0, 32.0]), 10, 7.5, 0.5, 1.5
    feats = U.build_case("edge-R")["feats"]  # CPU tensors: a launch would be refused too, but later and for another reason
    good = U.build_case("edge-R")["gt"]
    for bad_cls in (10.0, -1.0, 2.5, float("nan"), 1e9):
        gt = good.clone()
        gt[1, 2, 0] = bad_cls
        with pytest.raises(ValueError, match=r"class outside \[0, 10\)"):
            crit.from_gt(feats, gt)
    batch = {"batch_idx": torch.tensor([0.0, 1.0]), "cls": torch.tensor([[3.0], [10.0]]), "bboxes": torch.tensor([[0.5, 0.5, 0.2, 0.2], [0.4, 0.4, 0.1, 0.3]])}
    with pytest.raises(ValueError, match=r"class outside \[0, 10\)"):
        crit.targets_to_gt(batch, 2, (64, 64))
    batch["cls"][1] = 9.0
    assert crit.targets_to_gt(batch, 2, (64, 64)).shape == (2, 1, 5)
    v8DetectionLoss.check_classes(torch.zeros(2, 0, 5), 10)
